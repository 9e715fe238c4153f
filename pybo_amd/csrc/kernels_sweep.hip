// kernels_sweep.hip -- the acquisition sweep on gfx950.
//
// Replaces, for M candidates at once, what pybo reaches through `finit = f(xgrid, grad=False)`
// [pybo/solvers/lbfgs.py:50] -> index(X) [pybo/policies/simple.py:23-25,37-39,62-73] ->
// model.predict / get_improvement / get_tail (reggie, un-vendored), followed by
// `np.argsort(finit)[::-1]` [pybo/solvers/lbfgs.py:51] of which only the first nbest are used.
//
// Per chunk of candidate columns:
//   1. k_cross_gram   Ks[nt][k][c] = k(x_k, cand_{128 nt + c})    (HBM-write bound; tile-blocked so that every
//                     128-candidate column panel is one contiguous Np x 128 block)
//   2. k_sweep_trmm*  V = T Ks on fp64 MFMA, tile (mt, nt); V never leaves registers: the epilogue
//                     reduces colsum(V^2) and V^T a per 128-row block into Qp/Pp[mt][n]   (default: k_sweep_trmm_l -- operands by
//                     LDS-DMA, the zero rows of T's diagonal block skipped; the other schedules are bit-identical witnesses)
//   3. k_acq          q = sum_mt Qp, p = sum_mt Pp (fixed order -> deterministic),
//                     mu = bias + p, s2 = max(rho - q, S2_FLOOR), acquisition value   (cand_moments, acq_core.h)
// then one block-local + one merge top-k pass over all M values.
#include "acq_core_dev.h"
#include "gemm_core.h"
#include "gpx_internal.h"
#include "gpx_math.h"
#include "bound_exp.h"
#include "bound_f32.h"
#include "sweep_map.h"
#include "xgram_core.h"

namespace gpx {

// ------------------------------------------------------------------------------------------------
// cross-Gram: tile 64 observed rows x 128 candidate columns, 8x4 outputs per thread
// ------------------------------------------------------------------------------------------------
// (the tile's shape XK x XN, the coordinate chunk XDC and the distance arithmetic itself: xgram_core.h, shared with kernels_path.hip)

// One workgroup: 128 candidates x xrt consecutive 64-row tiles (the candidates' coordinates are staged once when
// d <= XDC).  grid (ceil(Np / 64 / xrt), cols / 128): consecutive workgroups write consecutive runs of Ks.
constexpr int XRT = 8;

template <int KID>
__global__ __launch_bounds__(256, 3) void k_cross_gram(const double* __restrict__ Xs, int64_t N, int64_t Np, int d,
                                                       const double* __restrict__ Xc, int64_t m0, int64_t M,
                                                       const double* __restrict__ invell, double rho,
                                                       double* __restrict__ Ks, int64_t ldk, int xrt) {
    __shared__ double xo[XDC][XK];
    __shared__ double xc[XDC][XN];
    const int t = threadIdx.x, tx = t & 31, ty = t >> 5;
    const int64_t n0 = (int64_t)blockIdx.y * XN;      // chunk-local candidate origin
    const bool onepass = (d <= XDC);
    if (onepass) xgram_stage_cand(xc, Xc, m0 + n0 + (t & (XN - 1)), M, d, invell, 0, d);
    for (int rt = 0; rt < xrt; ++rt) {
        const int64_t k0 = ((int64_t)blockIdx.x * xrt + rt) * XK;   // observed row origin
        if (k0 >= Np) break;
        double r2[8][4];
        xgram_tile_r2(xo, xc, Xs, k0, d, Xc, m0 + n0, M, invell, onepass, r2);
        // a tile without padding rows / columns (every tile of the north-star launch) needs no selects: two of the 58 VALU
        // instructions per entry of a kernel that is bound by their issue (workgroup-uniform branch)
        const bool full = (k0 + XK <= N) && (m0 + n0 + XN <= M);
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            const int64_t gk = k0 + ty * 8 + a;
            d4 o;
            if (full) {
#pragma unroll
                for (int b = 0; b < 4; ++b) o[b] = kern_eval(KID, r2[a][b], rho);
            } else {
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int64_t gm = m0 + n0 + tx * 4 + b;
                    o[b] = (gk < N && gm < M) ? kern_eval(KID, r2[a][b], rho) : 0.0;
                }
            }
            // tile-blocked layout [nt][k][128]: the 64 x 128 outputs of a row tile are ONE contiguous 64 KB run
            *reinterpret_cast<d4*>(Ks + ((int64_t)blockIdx.y * ldk + gk) * XN + tx * 4) = o;
        }
    }
}

// rows: the observed rows [0, rows) filled in every panel (a multiple of 128), at the pitch ldk -- the factor's Np for the sweep
// itself, the leading nR 128 <= N for the row-prefix pass of a selection-only sweep.  An entry's bits depend on its two points alone.
void launch_cross_gram(hipStream_t s, const double* Xs, int64_t rows, int64_t N, int d, const double* Xc,
                       int64_t m0, int64_t M, int64_t cols, const double* invell, int kernel_id,
                       double rho, double* Ks, int64_t ldk) {
    const int64_t Np = rows;
    const int64_t tiles = Np / XK;
    // row tiles per workgroup: the SE kernel at small d is bound by its 8 B/evaluation of stores (one tile per
    // workgroup interleaves them best: 3.5 vs 4.3 ms per 2^31 evaluations), the others by their VALU work (the
    // candidates staged once per 8 tiles: Matern-5/2 4.35 vs 4.85 ms); non-temporal stores change nothing
    const int XRTa = (kernel_id == GPX_KERN_SE_ARD && d <= XDC) ? 1 : XRT;       // (re-measured in round 6: SE 14.3 / 15.5 / 17.5 ms per 2^20 candidates with 1 / 2 / 4 tiles)
    const int XRTv = XRTa;
    dim3 grid((unsigned)((tiles + XRTa - 1) / XRTa), (unsigned)(cols / XN));   // x: row groups of one candidate tile = one contiguous run of Ks
#define GPX_CG(KID) \
    hipLaunchKernelGGL(k_cross_gram<KID>, grid, dim3(256), 0, s, Xs, N, Np, d, Xc, m0, M, invell, rho, Ks, ldk, XRTv)
    switch (kernel_id) {
        case GPX_KERN_SE_ARD: GPX_CG(GPX_KERN_SE_ARD); break;
        case GPX_KERN_MATERN52: GPX_CG(GPX_KERN_MATERN52); break;
        case GPX_KERN_MATERN32: GPX_CG(GPX_KERN_MATERN32); break;
        default: GPX_CG(GPX_KERN_MATERN12); break;
    }
#undef GPX_CG
}

// ------------------------------------------------------------------------------------------------
// THE dominant kernel: V(m,n) = sum_{k <= m} T(m,k) Ks(k,n),  T(m,k) = U[k][m]  (both k-major).
// Tile (mt, nt): 128 observed rows x 128 candidates, K-extent (mt+1)*128 (T is lower triangular),
// N^2 * M flop in total.  Heavy tiles (large mt) are dispatched first.
// ------------------------------------------------------------------------------------------------
// The block -> tile maps (sweep_tile_of) and the grid of a launch (sweep_grid): sweep_map.h.
// The summation order of a tile along k (the SAME in every schedule and every tile map: results stay bit-identical): tiles of the
// lower half, 2 mt < nP - 1 -- in the paired map exactly the SECOND tile of every pair -- take their 32-row k-steps downwards when
// the factor has at least 32 block rows.  In the paired map every workgroup of a super-tile then reads the same rows of its Ks
// panel at the same time in BOTH phases (row t in the first, row (nP + 1) 128 - t in the second, whatever its pair index), which
// lets an XCD's L2 serve the panel once: L2 -> fabric reads 101 -> 88 GB per launch at N = 8192 and, the kernel being power-bound,
// 0.8 % more clock on the boxes that sustain 2300 MHz (nothing on those at 2385) -- profiles/r06_sweep_power_probes.txt.  Below 32
// block rows the second tiles are short and it costs 0.3 %.
__device__ __forceinline__ bool sweep_tile_rev(int mt, int nP) { return nP >= 32 && 2 * mt < nP - 1; }

// epilogue of a tile: column sums of V^2 and V*a over its 128 rows -> Qp / Pp[mt][n0 ..] (red: 512 doubles of LDS, free)
// NJ < 4: a narrow tile (gemm_tile_128_l): 32 NJ columns, wave (wm, wn) holds columns 16 NJ wn + 16 j.  A column's sums are formed
// from its own accumulator column by its own two waves in the wide tile's order, so they are the wide tile's bits.
template <bool ILV = false, int NJ = 4>
__device__ __forceinline__ void sweep_epilogue(const d4 (&acc)[4][NJ], const double* __restrict__ avec, int64_t m0,
                                               double* __restrict__ Qrow, double* __restrict__ Prow, double* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int wm = w >> 1, wn = w & 1;
    double qs[NJ] = {}, ps[NJ] = {};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double av[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) av[r] = avec[m0 + (ILV ? (2 * i + wm) * 16 : wm * 64 + i * 16) + (lane >> 4) + 4 * r];
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double v = acc[i][j][r];
                qs[j] = fma(v, v, qs[j]);
                ps[j] = fma(v, av[r], ps[j]);
            }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        double q = qs[j], p = ps[j];
        q += __shfl_xor(q, 16);
        p += __shfl_xor(p, 16);
        q += __shfl_xor(q, 32);
        p += __shfl_xor(p, 32);
        qs[j] = q;
        ps[j] = p;
    }
    if (lane < 16) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = wn * (16 * NJ) + j * 16 + lane;
            red[(wm * TB + c) * 2 + 0] = qs[j];
            red[(wm * TB + c) * 2 + 1] = ps[j];
        }
    }
    __syncthreads();
    if (threadIdx.x < 32 * NJ) {
        const int c = threadIdx.x;
        Qrow[c] = red[c * 2] + red[(TB + c) * 2];
        Prow[c] = red[c * 2 + 1] + red[(TB + c) * 2 + 1];
    }
}

// The frame of every schedule of the dominant kernel: the workgroup's tile (or tile pair) from the map, per tile the operand
// pointers, the K-extent and the up/down rule, the k-loop `loop(acc, At, Bt, kend, rev)` of the schedule, the epilogue.
// (interleaved row blocks in every schedule: the column sums then add a tile's rows in the same order everywhere)
// Np is the leading dimension of U, the panel pitch of Ks and, as nP, the factor's block rows of the up/down rule; nR <= nP is the
// number of block rows the map covers.  A tile's arithmetic depends on its rows of U, its panel, its K-extent and the rule -- not
// on nR: a row-prefix launch (nR < nP) writes into Qp / Pp[mt < nR] the very bits the full launch (nR = nP) writes there.
// NJ < 4: NARROW tiles of 128 rows x W = 32 NJ candidates (the default schedule only): NT counts narrow tiles, tile nt is columns
// [nt W, nt W + W) of panel nt W / 128 and writes the Qp / Pp entries of those columns.  Per wave the rows (ILV), the k-step order,
// the TRI skip, the up/down rule and the sequence of MFMAs along k of every accumulator block are those of the wide tile, and no
// column of a tile enters another column's sums (gemm_tile_128_l, sweep_epilogue): a launch writes the same bits at every width.
template <int RES, int NJ = 4, class Loop>
__device__ __forceinline__ void sweep_tiles(int b, const double* __restrict__ U, int64_t Np, const double* __restrict__ Ks, int NT,
                                            int nR, const double* __restrict__ avec, double* __restrict__ Qp, double* __restrict__ Pp,
                                            int64_t ldp, int order, int sm, unsigned long long* clk, double* smem, Loop loop) {
    const LaunchClock lc;
    const int nP = (int)(Np / TB);
    int mt, nt, mt2;
    if (!sweep_tile_of<RES>(b, order, sm, NT, nR, mt, nt, mt2)) return;
#pragma unroll 1
    for (int ph = 0; ph < 2; ++ph) {
        if (ph == 1) {
            if (mt2 < 0) break;
            mt = mt2;
            __syncthreads();               // the epilogue's LDS reads are done before the next tile stages
        }
        const int64_t m0 = (int64_t)mt * TB, n0 = (int64_t)nt * (32 * NJ);
        d4 acc[4][NJ];
        acc_zero(acc);
        loop(acc, U + m0, Ks + (n0 / TB) * Np * TB, (mt + 1) * TB, sweep_tile_rev(mt, nP), (int)(n0 % TB));
        // the k-loop ended on a barrier, LDS is free
        sweep_epilogue<true, NJ>(acc, avec, m0, Qp + (int64_t)mt * ldp + n0, Pp + (int64_t)mt * ldp + n0, smem);
    }
    lc.add(clk);
}

// The register-staged schedules of rounds 1 (VAR 2), 2 (5) and 5 (6).
template <int VAR>
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_sweep_trmm(const double* __restrict__ U, int64_t Np,
                                                                const double* __restrict__ Ks,
                                                                int64_t ldk, int NT, int nR,
                                                                const double* __restrict__ avec,
                                                                double* __restrict__ Qp,
                                                                double* __restrict__ Pp, int64_t ldp,
                                                                int order, int sm, unsigned long long* clk) {
    __shared__ __attribute__((aligned(16))) double smem[GEMM_LDS_F64];
    sweep_tiles<64>(blockIdx.x, U, Np, Ks, NT, nR, avec, Qp, Pp, ldp, order, sm, clk, smem,
                    [&](d4 (&acc)[4][4], const double* At, const double* Bt, int kend, bool rev, int) {
        if (!rev) {
            if (VAR == 2) gemm_tile_128_b<true, true>(acc, At, Np, Bt, TB, 0, kend, smem);
            else if (VAR == 5) gemm_tile_128_g<1, false, true>(acc, At, Np, Bt, TB, 0, kend, smem);
            else gemm_tile_128_s<1, false, true>(acc, At, Np, Bt, TB, 0, kend, smem);
        } else {
            if (VAR == 2) gemm_rev32(0, kend, [&](int k0, int k1) { gemm_tile_128_b<true, true>(acc, At, Np, Bt, TB, k0, k1, smem); });
            else if (VAR == 5) gemm_tile_128_g<1, false, true, true>(acc, At, Np, Bt, TB, 0, kend, smem);
            else gemm_tile_128_s<1, false, true, true>(acc, At, Np, Bt, TB, 0, kend, smem);
        }
    });
}

// The same tiles through the register-free k-loop (gemm_tile_128_l): WGS workgroups per compute unit.
// TRI: the all-zero quarter-rows of T's diagonal block are skipped (1.5 of 4 k-steps of every tile).
// DOWN = false: every tile upwards (probe builds only: the A/B of the order rule -- NOT bit-identical with the shipped schedules)
// NJ = 2, 1: narrow tiles of 64 / 32 candidates (sweep_tiles), for launches of few candidates over long factors: a workgroup's k-chain
// is as long as the wide tile's but a k-step holds a half / a quarter of its MFMAs, and the launch has 2 / 4 times the workgroups.
template <int BKL, int WGS, int PRIO, int NSET, bool TRI, int AUX = 0, bool DOWN = true, int NJ = 4>
__global__ __launch_bounds__(GEMM_THREADS, WGS) void k_sweep_trmm_l(const double* __restrict__ U, int64_t Np,
                                                                    const double* __restrict__ Ks, int64_t ldk, int NT, int nR,
                                                                    const double* __restrict__ avec,
                                                                    double* __restrict__ Qp, double* __restrict__ Pp,
                                                                    int64_t ldp, int order, int sm,
                                                                    unsigned long long* clk, int b0) {
    __shared__ __attribute__((aligned(16))) double smem[gemm_l_lds_f64<BKL>()];
    static_assert(NJ == 4 || BKL == 32, "narrow tiles: the 32-row k-step only");
    sweep_tiles<32 * WGS, NJ>((int)blockIdx.x + b0, U, Np, Ks, NT, nR, avec, Qp, Pp, ldp, order, sm, clk, smem,
                              [&](d4 (&acc)[4][NJ], const double* At, const double* Bt, int kend, bool rev, int bcol) {
        if (!(DOWN && rev)) gemm_tile_128_l<BKL, PRIO, NSET, true, TRI, false, AUX>(acc, At, Np, Bt, TB, 0, kend, smem, bcol);
        else if constexpr (BKL == 32) gemm_tile_128_l<32, PRIO, NSET, true, TRI, false, AUX, true>(acc, At, Np, Bt, TB, 0, kend, smem, bcol);
        else gemm_rev32(0, kend, [&](int k0, int k1) { gemm_tile_128_l<BKL, PRIO, NSET, true, false, false, AUX>(acc, At, Np, Bt, TB, k0, k1, smem); });
    });
}

// The default schedule for a launch with at most one working workgroup per compute unit (sweep_shape_of: images = 2): the same tiles,
// wide or narrow, through gemm_tile_128_l2 -- two k-step images, the next step's DMA behind this step's MFMAs, one barrier per step.
// ONE workgroup per CU (2 x 73,728 B of dynamic LDS), so the map's RES is 32.  FG: gemm_tile_128_l2 (probe builds vary it).
// (launch bounds of TWO workgroups per CU although LDS admits one: with one the compiler keeps the accumulators in AGPRs and copies
//  all of them to VGPRs and back around every k-step; the register budget of two keeps them in VGPRs as in k_sweep_trmm_l.)
template <int NSET, int NJ, int FG = (NJ == 1 ? 1 : 4)>
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_sweep_trmm_l2(const double* __restrict__ U, int64_t Np,
                                                                   const double* __restrict__ Ks, int64_t ldk, int NT, int nR,
                                                                   const double* __restrict__ avec,
                                                                   double* __restrict__ Qp, double* __restrict__ Pp,
                                                                   int64_t ldp, int order, int sm,
                                                                   unsigned long long* clk, int b0) {
    extern __shared__ __attribute__((aligned(16))) double sweep_l2_smem[];
    sweep_tiles<32, NJ>((int)blockIdx.x + b0, U, Np, Ks, NT, nR, avec, Qp, Pp, ldp, order, sm, clk, sweep_l2_smem,
                        [&](d4 (&acc)[4][NJ], const double* At, const double* Bt, int kend, bool rev, int bcol) {
        if (!rev) gemm_tile_128_l2<1, NSET, true, true, false, 0, false, NJ, FG>(acc, At, Np, Bt, TB, 0, kend, sweep_l2_smem, bcol);
        else gemm_tile_128_l2<1, NSET, true, true, false, 0, true, NJ, FG>(acc, At, Np, Bt, TB, 0, kend, sweep_l2_smem, bcol);
    });
}
constexpr int SWEEP_L2_LDS_BYTES = 2 * gemm_l_lds_f64<32>() * 8;
#ifdef GPX_SWEEP_PROBES
static int g_sweep_probe_fg = 0;   // 0: the library's FG
#endif

// The same tiles on the barrier-free loop (gemm_tile_128_w: every wave fetches its own operand halves, one 16-row image per
// wave, two workgroups per CU), with the diagonal block's zero rows skipped.  Twice the L2 -> LDS bytes of k_sweep_trmm_l.
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_sweep_trmm_w(const double* __restrict__ U, int64_t Np,
                                                                  const double* __restrict__ Ks, int64_t ldk, int NT, int nR,
                                                                  const double* __restrict__ avec, double* __restrict__ Qp,
                                                                  double* __restrict__ Pp, int64_t ldp, int order, int sm,
                                                                  unsigned long long* clk) {
    __shared__ __attribute__((aligned(16))) double smem[4 * GEMM_W_IMG_F64];
    sweep_tiles<64>(blockIdx.x, U, Np, Ks, NT, nR, avec, Qp, Pp, ldp, order, sm, clk, smem,
                    [&](d4 (&acc)[4][4], const double* At, const double* Bt, int kend, bool rev, int) {
        if (!rev) gemm_tile_128_w<1, 1, false, true, 0, true>(acc, At, Np, Bt, TB, 0, kend, smem);
        else gemm_rev32(0, kend, [&](int k0, int k1) { gemm_tile_128_w<1, 1, false, true, 0, false>(acc, At, Np, Bt, TB, k0, k1, smem); });
    });
}

// The map of a launch (sweep_order_of) and the shape of its tiles (sweep_shape_of: width and LDS images of the default schedule, by
// the options or by size): sweep_map.h.

// the compute units of the current device (the by-size rule of sweep_shape_of), asked for once per device
static int device_cus() {
    static int cus[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    if (!cus[dev]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return 0;
        cus[dev] = n;
    }
    return cus[dev];
}

// nR: the block rows [0, nR) the launch covers -- the factor's Np / 128 for the sweep itself, fewer for the row-prefix pass of a
// selection-only sweep (api.hip: second_bound, step 4a), which needs rows [0, nR 128) of every Ks panel only.
void launch_sweep_trmm(hipStream_t s, const double* U, int64_t Np, int nR, const double* Ks, int64_t ldk,
                       int64_t cols, const double* a, double* Qp, double* Pp, int64_t ldp,
                       int tile_order, int super_m, unsigned long long* clk, int short_map, int64_t valid, int sweep_cols, int sweep_images) {
    const int NT = (int)(cols / TB);
    if (valid < 0 || valid > cols) valid = cols;
    const SweepShape shape = sweep_shape_of(tile_order, (int)(Np / TB), nR, valid, sweep_images < 0 ? device_cus() : 0, sweep_cols, sweep_images,
                                            super_m, short_map);
    // bits 0-1: tile map, bits 2-4: k-loop (4 = default: operands by LDS-DMA, k-step 32, two workgroups per CU, the zero rows of
    // T's diagonal block skipped; 3: the same without the skip; 1: the barrier-free wave-private loop; 7: k-step 16, three workgroups per CU; 6, 5, 2: the
    // register-staged schedules of rounds 5, 2, 1 -- all kept as independently scheduled witnesses of the bit-identity test)
    // short_map (option "short_map"): map 3 takes its short form (sweep_map.h) -1 where the launch cannot fill the per-XCD patches,
    // 0 never, 1 always; 2 the strided short form (scripts/probe/sweep_ab.hip only: gpx_set_option admits -1 .. 1)
    const int order0 = tile_order & 3, var = (tile_order >> 2) & 7;
#define GPX_SW(K) hipLaunchKernelGGL(K, dim3(nblk), dim3(GEMM_THREADS), 0, s, U, Np, Ks, ldk, NT, nR, a, Qp, Pp, ldp, order, super_m, clk)
#define GPX_SWL(K) hipLaunchKernelGGL(K, dim3(nblk), dim3(GEMM_THREADS), 0, s, U, Np, Ks, ldk, NT, nR, a, Qp, Pp, ldp, order, super_m, clk, 0)
    if (var == 7) {                // three workgroups per CU, k-step 16
        const int order = sweep_order_of<96>(order0, short_map, super_m, NT);
        const unsigned nblk = sweep_grid<96>(order, super_m, NT, nR);
        GPX_SWL((k_sweep_trmm_l<16, 3, 1, 2, false>));
    } else if (var == 1) {               // barrier-free: every wave keeps its own operands
        const int order = sweep_order_of<64>(order0, short_map, super_m, NT);
        const unsigned nblk = sweep_grid<64>(order, super_m, NT, nR);
        GPX_SW(k_sweep_trmm_w);
    } else if (shape.images == 2) {
        // the default schedule, one workgroup per CU on two LDS images: the same maps (32 workgroups resident per XCD) over NTn tiles of W columns
        const int W = shape.width;
        const int NTn = (int)((valid + W - 1) / W);
        const int order = sweep_order_of<32>(order0, short_map, super_m, NTn);
        const unsigned nblk = sweep_grid<32>(order, super_m, NTn, nR);
#define GPX_SW2(K)                                                                                                        \
    do {                                                                                                                  \
        hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, SWEEP_L2_LDS_BYTES);              \
        hipLaunchKernelGGL(K, dim3(nblk), dim3(GEMM_THREADS), SWEEP_L2_LDS_BYTES, s, U, Np, Ks, ldk, NTn, nR, a, Qp, Pp, ldp, order, super_m, clk, 0); \
    } while (0)
#ifdef GPX_SWEEP_PROBES          // scripts/probe/sweep_ab.hip only: the pieces the next step's DMA goes out in (gemm_tile_128_l2: FG)
        const int fg = (int)g_sweep_probe_fg;
        if (W == 32 && fg == 2) GPX_SW2((k_sweep_trmm_l2<2, 1, 2>));
        else if (W == 32 && fg == 4) GPX_SW2((k_sweep_trmm_l2<2, 1, 4>));
        else if (W == 64 && fg == 2) GPX_SW2((k_sweep_trmm_l2<2, 2, 2>));
        else if (W == 64 && fg == 1) GPX_SW2((k_sweep_trmm_l2<2, 2, 1>));
        else if (W == 128 && fg == 1) GPX_SW2((k_sweep_trmm_l2<2, 4, 1>));
        else
#endif
        if (W == 32) GPX_SW2((k_sweep_trmm_l2<2, 1>));
        else if (W == 64) GPX_SW2((k_sweep_trmm_l2<2, 2>));
        else GPX_SW2((k_sweep_trmm_l2<2, 4>));
#undef GPX_SW2
    } else if (const int W = shape.width; W < TB) {
        // the default schedule on narrow tiles: the same maps over NTn tiles of W columns
        const int NTn = (int)((valid + W - 1) / W);
        const int order = sweep_order_of<64>(order0, short_map, super_m, NTn);
        const unsigned nblk = sweep_grid<64>(order, super_m, NTn, nR);
#define GPX_SWN(K) hipLaunchKernelGGL(K, dim3(nblk), dim3(GEMM_THREADS), 0, s, U, Np, Ks, ldk, NTn, nR, a, Qp, Pp, ldp, order, super_m, clk, 0)
        if (W == 64) GPX_SWN((k_sweep_trmm_l<32, 2, 1, 2, true, 0, true, 2>));
        else GPX_SWN((k_sweep_trmm_l<32, 2, 1, 2, true, 0, true, 1>));
#undef GPX_SWN
    } else if (var == 4 || var == 3) {   // two workgroups per CU, k-step 32; 4: with the diagonal block's zero rows skipped
        const int order = sweep_order_of<64>(order0, short_map, super_m, NT);
        const unsigned nblk = sweep_grid<64>(order, super_m, NT, nR);
#ifdef GPX_SWEEP_PROBES          // scripts/probe/sweep_ab.hip only: variants that are NOT schedules of the library (profiles/r06_sweep_power_probes.txt)
        const int aux = tile_order >> 5;         // (probe builds only: cache policy of the operand loads; gpx_set_option admits 0)
        if (var == 4 && aux == 1) GPX_SWL((k_sweep_trmm_l<32, 2, 1, 2, true, 1>));
        else if (var == 4 && aux == 2) GPX_SWL((k_sweep_trmm_l<32, 2, 1, 2, true, 2>));
        else if (var == 4 && aux == 3) GPX_SWL((k_sweep_trmm_l<32, 2, 1, 2, true, 16>));
        else if (var == 4 && aux == 4) GPX_SWL((k_sweep_trmm_l<32, 2, 1, 2, true, 17>));
        else if (var == 4 && aux == 5) GPX_SWL((k_sweep_trmm_l<32, 2, 1, 2, true, 3>));
        else if (var == 4 && aux == 6) GPX_SWL((k_sweep_trmm_l<32, 2, 1, 2, true, 0, false>));      // every tile upwards (round 6's first form)
        else if (var == 4 && aux == 7) {        // probe: one launch per generation of 512 workgroups (every generation starts aligned)
            for (unsigned g0 = 0; g0 < nblk; g0 += 512)
                hipLaunchKernelGGL((k_sweep_trmm_l<32, 2, 1, 2, true>), dim3(nblk - g0 < 512 ? nblk - g0 : 512), dim3(GEMM_THREADS), 0, s, U, Np, Ks, ldk, NT, nR, a,
                                   Qp, Pp, ldp, order, super_m, clk, (int)g0);
        }
        else
#endif
        if (var == 4) GPX_SWL((k_sweep_trmm_l<32, 2, 1, 2, true>));
        else GPX_SWL((k_sweep_trmm_l<32, 2, 1, 2, false>));
    } else {
        const int order = sweep_order_of<64>(order0, short_map, super_m, NT);
        const unsigned nblk = sweep_grid<64>(order, super_m, NT, nR);
        if (var == 2) GPX_SW(k_sweep_trmm<2>);
        else if (var == 6) GPX_SW(k_sweep_trmm<6>);
        else GPX_SW(k_sweep_trmm<5>);
    }
#undef GPX_SW
#undef GPX_SWL
}

// ------------------------------------------------------------------------------------------------
// acquisition values from the reduced partials (one thread per candidate; coalesced over n)
// ------------------------------------------------------------------------------------------------
// (norm_cdf, norm_pdf and acq_value, the ONE place the acquisition arithmetic lives: gpx_math.h -- kernels_batch.hip scores with them too)

// nrb > 0: Qp/Pp are per-row-block partials (nrb, ldp) of this chunk, reduced in block order.
// nrb = 0: Qp/Pp are the already reduced per-candidate sums of the whole grid (the sweep cache), m0 = 0.
// qsum/psum (optional): the reduced sums are stored per candidate (warm BO step).  acq_frame (acq_core_dev.h) with acq_value as its
// scoring step; k_acq_mes (kernels_mes.hip) is the same frame with another one.
__global__ __launch_bounds__(256) void k_acq(const double* __restrict__ Qp, const double* __restrict__ Pp,
                                             int64_t ldp, int nrb, int64_t m0, int64_t cols_valid,
                                             double rho, double bias, int acq_id, double p0,
                                             double* __restrict__ acq_out, double* __restrict__ mu_out,
                                             double* __restrict__ s2_out, double* __restrict__ qsum,
                                             double* __restrict__ psum) {
    acq_frame(Qp, Pp, ldp, nrb, m0, cols_valid, rho, bias, [=](double mu, double s2) { return acq_value(acq_id, mu, s2, p0); }, acq_out,
              mu_out, s2_out, qsum, psum);
}

void launch_acq(hipStream_t s, const double* Qp, const double* Pp, int64_t ldp, int nrb, int64_t m0,
                int64_t cols_valid, double rho, double bias, int acq_id, double p0, double* acq_out,
                double* mu_out, double* s2_out, double* qsum, double* psum) {
    const unsigned g = (unsigned)((cols_valid + 255) / 256);
    hipLaunchKernelGGL(k_acq, dim3(g), dim3(256), 0, s, Qp, Pp, ldp, nrb, m0, cols_valid, rho, bias,
                       acq_id, p0, acq_out, mu_out, s2_out, qsum, psum);
}

// ------------------------------------------------------------------------------------------------
// Warm BO step: correction of the cached per-candidate sums after q appended observations (q <= Q).
// With w_j = K_j^-1 k(X_j, x_j) (K_j, X_j: the model just before point j was appended), d_j the posterior std of
// observation j (incl. noise) and a_j the new entry of a:
//     v_jn = ( k(x_j, z_n) - sum_{i < N_j} w_ji k(x_i, z_n) ) / d_j        (the new row j of V = T K*)
//     q_n += sum_j v_jn^2          p_n += sum_j v_jn a_j
// i.e. ONE pass of N*M covariance evaluations with q fused row-dots instead of the N^2 M triangular product --
// what `model.add_data(x, y)` + the next `index(xgrid)` cost in the reference is a full refit and a full solve
// (pybo/bayesopt.py:269, pybo/solvers/lbfgs.py:50).  The q points of one `add_data(X, Y)` call share the pass:
// the covariance evaluations dominate (46 fp64 instructions each against one FMA per extra point).
// Wq (q, ldw): row j = [w_j (N_j entries), -1 at position N_j (the point's own row of Xs), zeros], so that
// v_jn = - (Wq_j . k(X_all, z_n)) / d_j with one dot over all Ntot = N_0 + q rows.  pscal (q, 2) = {1/d_j, a_j}.
// One workgroup owns 128 candidates and walks all observed rows in tiles of 64 (fixed order: results do not
// depend on the launch geometry); thread (ty, tx) accumulates rows ty*8..+7 of each tile for candidates
// tx*4..+3, the 8 row groups are combined through LDS at the end.
// ------------------------------------------------------------------------------------------------
template <int Q, int KID>
__global__ __launch_bounds__(256, (Q == 1) ? 3 : 2) void k_sweep_rankq(const double* __restrict__ Xs, int64_t Ntot, int d,
                                                     const double* __restrict__ Wq, int64_t ldw, int q,
                                                     const double* __restrict__ pscal,
                                                     const double* __restrict__ Z, int64_t M,
                                                     const double* __restrict__ invell, double rho,
                                                     double* __restrict__ qsum, double* __restrict__ psum,
                                                     const double* __restrict__ xlast, double* __restrict__ vout,
                                                     const double* __restrict__ skip) {
    // skip (optional, the bound pass of a selection-only sweep): *skip == 1.0 says k_bound_mfma has written vout -- nothing to do.
    if (skip && *skip == 1.0) return;
    // xlast (optional): the scaled coordinates of row Ntot - 1 when that row is NOT in Xs yet -- an ANNOUNCED
    // observation (gpx_append_begin): its location is known, its value is not, the factor is untouched.
    // vout (optional, q == 1): write v_n instead of updating the sums; gpx_append applies q += v^2, p += v a once the
    // value has arrived (k_cache_apply: the same two FMAs, the same bits).
    __shared__ double xo[XDC][XK];
    __shared__ double xc[XDC][XN];
    __shared__ double wv[Q][XK];
    __shared__ double red[8][XN];
    const int t = threadIdx.x, tx = t & 31, ty = t >> 5;
    const int64_t n0 = (int64_t)blockIdx.x * XN;
    double acc[Q][4];
#pragma unroll
    for (int j = 0; j < Q; ++j)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[j][b] = 0.0;
    const bool onepass = (d <= XDC);          // candidates' coordinates stay in LDS across row tiles
    const int crow = t & (XN - 1), ckq = t >> 7;      // staging of candidates: row, first coordinate (stride 2)
    const int orow = t & (XK - 1), okq = t >> 6;      // staging of observed rows: row, first coordinate (stride 4)
    const int64_t gmc = n0 + crow;
    if (onepass)
        for (int k = ckq; k < d; k += 2) xc[k][crow] = (gmc < M) ? Z[gmc * d + k] * invell[k] : 0.0;
    for (int64_t k0 = 0; k0 < Ntot; k0 += XK) {
        double r2[8][4];
        auto stage = [&](int c0, int kc) {
            __syncthreads();
            const int64_t gr = k0 + orow;
            const double* src = (xlast && gr == Ntot - 1) ? xlast + c0 : Xs + gr * d + c0;
            for (int k = okq; k < kc; k += 4) xo[k][orow] = (gr < Ntot) ? src[k] : 0.0;
            if (c0 == 0) {
                for (int e = t; e < Q * XK; e += 256) {
                    const int j = e / XK, row = e - j * XK;      // XK is a compile-time power of two
                    wv[j][row] = (j < q && k0 + row < Ntot) ? Wq[(int64_t)j * ldw + k0 + row] : 0.0;
                }
            }
            if (!onepass)
                for (int k = ckq; k < kc; k += 2)
                    xc[k][crow] = (gmc < M) ? Z[gmc * d + c0 + k] * invell[c0 + k] : 0.0;
            __syncthreads();
        };
        {
            const int kc = min(XDC, d);
            stage(0, kc);
            dist_step<true>(xo, xc, 0, ty, tx, r2);
#pragma unroll 1
            for (int k = 1; k < kc; ++k) dist_step<false>(xo, xc, k, ty, tx, r2);
        }
        for (int c0 = XDC; c0 < d; c0 += XDC) {
            const int kc = min(XDC, d - c0);
            stage(c0, kc);
#pragma unroll 1
            for (int k = 0; k < kc; ++k) dist_step<false>(xo, xc, k, ty, tx, r2);
        }
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            double kv[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) kv[b] = kern_eval(KID, r2[a][b], rho);
#pragma unroll
            for (int j = 0; j < Q; ++j) {
                const double wa = wv[j][ty * 8 + a];      // 0 beyond a point's own row: contributes nothing
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[j][b] = fma(wa, kv[b], acc[j][b]);
            }
        }
    }
    double dq = 0.0, dp = 0.0;
#pragma unroll
    for (int j = 0; j < Q; ++j) {
        __syncthreads();
#pragma unroll
        for (int b = 0; b < 4; ++b) red[ty][tx * 4 + b] = acc[j][b];
        __syncthreads();
        if (t < XN && j < q) {
            double dot = 0.0;
#pragma unroll
            for (int g = 0; g < 8; ++g) dot += red[g][t];
            const double v = -dot * pscal[2 * j];
            if (vout) {
                if (n0 + t < M) vout[n0 + t] = v;
            } else {
                dq = fma(v, v, dq);
                dp = fma(v, pscal[2 * j + 1], dp);
            }
        }
    }
    if (t < XN && !vout) {
        const int64_t gm = n0 + t;
        if (gm < M) {
            qsum[gm] += dq;
            psum[gm] += dp;
        }
    }
}

// the value of an announced observation has arrived: q_n += v_n^2, p_n += v_n a  (a = scal[2], device-resident)
__global__ void k_cache_apply(const double* __restrict__ v, const double* __restrict__ scal, int64_t M,
                              double* __restrict__ qsum, double* __restrict__ psum) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const double vi = v[i];
    qsum[i] += fma(vi, vi, 0.0);
    psum[i] += fma(vi, scal[2], 0.0);
}

void launch_cache_apply(hipStream_t s, const double* v, const double* scal, int64_t M, double* qsum, double* psum) {
    hipLaunchKernelGGL(k_cache_apply, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, v, scal, M, qsum, psum);
}

// x scaled by 1/ell (the row an announced observation will occupy in Xs)
__global__ void k_scale_point(const double* __restrict__ x, const double* __restrict__ invell, int d,
                              double* __restrict__ xs) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < d) xs[k] = x[k] * invell[k];
}

void launch_scale_point(hipStream_t s, const double* x, const double* invell, int d, double* xs) {
    hipLaunchKernelGGL(k_scale_point, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, s, x, invell, d, xs);
}

template <int Q>
static void launch_rankq_kid(hipStream_t s, dim3 grid, const double* Xs, int64_t Ntot, int d, const double* Wq,
                             int64_t ldw, int q, const double* pscal, const double* Z, int64_t M, const double* invell,
                             int kernel_id, double rho, double* qsum, double* psum, const double* xlast, double* vout,
                             const double* skip = nullptr) {
#define GPX_RANKQ(KID)                                                                                              \
    hipLaunchKernelGGL((k_sweep_rankq<Q, KID>), grid, dim3(256), 0, s, Xs, Ntot, d, Wq, ldw, q, pscal, Z, M, invell, \
                       rho, qsum, psum, xlast, vout, skip)
    switch (kernel_id) {
        case GPX_KERN_SE_ARD: GPX_RANKQ(GPX_KERN_SE_ARD); break;
        case GPX_KERN_MATERN52: GPX_RANKQ(GPX_KERN_MATERN52); break;
        case GPX_KERN_MATERN32: GPX_RANKQ(GPX_KERN_MATERN32); break;
        default: GPX_RANKQ(GPX_KERN_MATERN12); break;
    }
#undef GPX_RANKQ
}

// the correction pass of ONE announced observation: v_n for every cached candidate -> vout (sums untouched)
void launch_sweep_rank1_v(hipStream_t s, const double* Xs, int64_t Ntot, int d, const double* Wq, int64_t ldw,
                          const double* pscal, const double* Z, int64_t M, const double* invell, int kernel_id,
                          double rho, const double* xlast, double* vout, const double* skip) {
    const dim3 grid((unsigned)((M + XN - 1) / XN));
    launch_rankq_kid<1>(s, grid, Xs, Ntot, d, Wq, ldw, 1, pscal, Z, M, invell, kernel_id, rho, nullptr, nullptr, xlast,
                        vout, skip);
}

// row j of the pending-correction table: [w (Nj entries), -1, zeros up to ldw]; pscal_j = {1/d, a_new}
__global__ void k_pend_store(const double* __restrict__ w, int64_t Nj, int64_t ldw, const double* __restrict__ scal,
                             double* __restrict__ row, double* __restrict__ pscal_j) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < ldw) row[i] = (i < Nj) ? w[i] : ((i == Nj) ? -1.0 : 0.0);
    if (i == 0) {
        pscal_j[0] = scal[1];
        pscal_j[1] = scal[2];
    }
}

void launch_pend_store(hipStream_t s, const double* w, int64_t Nj, int64_t ldw, const double* scal, double* row,
                       double* pscal_j) {
    hipLaunchKernelGGL(k_pend_store, dim3((unsigned)((ldw + 255) / 256)), dim3(256), 0, s, w, Nj, ldw, scal, row,
                       pscal_j);
}

void launch_sweep_rankq(hipStream_t s, const double* Xs, int64_t Ntot, int d, const double* Wq, int64_t ldw, int q,
                        const double* pscal, const double* Z, int64_t M, const double* invell, int kernel_id,
                        double rho, double* qsum, double* psum) {
    const dim3 grid((unsigned)((M + XN - 1) / XN));
    if (q == 1)
        launch_rankq_kid<1>(s, grid, Xs, Ntot, d, Wq, ldw, q, pscal, Z, M, invell, kernel_id, rho, qsum, psum, nullptr,
                            nullptr);
    else if (q <= 4)
        launch_rankq_kid<4>(s, grid, Xs, Ntot, d, Wq, ldw, q, pscal, Z, M, invell, kernel_id, rho, qsum, psum, nullptr,
                            nullptr);
    else
        launch_rankq_kid<8>(s, grid, Xs, Ntot, d, Wq, ldw, q, pscal, Z, M, invell, kernel_id, rho, qsum, psum, nullptr,
                            nullptr);
}

// ------------------------------------------------------------------------------------------------
// top-k: value descending, ties -> lower index; NaN ranks below everything (the order and its block_argmax: acq_core.h, acq_core_dev.h)
// ------------------------------------------------------------------------------------------------

// cutv / cuti (optional, device): only candidates that rank strictly AFTER the pair (*cutv, *cuti) take part -- the
// k-th best of an earlier pass: requests beyond TOPK_PASS entries are served TOPK_PASS at a time (launch_topk).
__global__ __launch_bounds__(256) void k_topk_block(const double* __restrict__ vals, int64_t M, int k,
                                                    double* __restrict__ blkv,
                                                    int64_t* __restrict__ blki, const double* __restrict__ cutv,
                                                    const int64_t* __restrict__ cuti) {
    __shared__ double sv[4];
    __shared__ int64_t si[4];
    // blockIdx.y: one of several value rows ranked by the same launch (the draws of a Thompson sweep): row q's values start
    // at vals + q M, its block lists at blkv / blki + q gridDim.x k
    vals += (int64_t)blockIdx.y * M;
    blkv += (int64_t)blockIdx.y * gridDim.x * k;
    blki += (int64_t)blockIdx.y * gridDim.x * k;
    const int64_t base = (int64_t)blockIdx.x * TK_PER_BLOCK;
    const bool cut = cutv != nullptr;
    const double cv = cut ? *cutv : 0.0;
    const int64_t ci = cut ? *cuti : 0;
    double v[TK_PER_THREAD];
#pragma unroll
    for (int e = 0; e < TK_PER_THREAD; ++e) {
        const int64_t idx = base + e * 256 + threadIdx.x;
        v[e] = nan_last((idx < M) ? vals[idx] : NEG_INF);
    }
    unsigned used = 0;  // bit e set: element e already emitted (or ranked at / before the cut)
    if (cut) {
#pragma unroll
        for (int e = 0; e < TK_PER_THREAD; ++e) {
            const int64_t idx = base + e * 256 + threadIdx.x;
            // (ci < 0: the earlier pass already ran out of candidates -- its last entry is the -1 marker: nothing is left)
            if (ci < 0 || !better(cv, ci, v[e], idx)) used |= 1u << e;
        }
    }
    for (int it = 0; it < k; ++it) {
        double bv = NEG_INF;
        int64_t bi = IDX_NONE;
#pragma unroll
        for (int e = 0; e < TK_PER_THREAD; ++e) {
            const int64_t idx = base + e * 256 + threadIdx.x;
            if (!((used >> e) & 1u) && idx < M && better(v[e], idx, bv, bi)) { bv = v[e]; bi = idx; }
        }
        block_argmax(bv, bi, sv, si);
        if (bi != IDX_NONE) {
            const int64_t off = bi - base;
            if ((int)(off & 255) == (int)threadIdx.x) used |= 1u << (unsigned)(off >> 8);
        }
        if (threadIdx.x == 0) {
            blkv[(int64_t)blockIdx.x * k + it] = bv;
            blki[(int64_t)blockIdx.x * k + it] = bi;
        }
    }
}

__global__ __launch_bounds__(256) void k_topk_merge(double* __restrict__ blkv, int64_t* __restrict__ blki,
                                                    int64_t n, int k, double* __restrict__ topv,
                                                    int64_t* __restrict__ topi) {
    __shared__ double sv[4];
    __shared__ int64_t si[4];
    blkv += (int64_t)blockIdx.x * n;          // blockIdx.x: the value row (see k_topk_block)
    blki += (int64_t)blockIdx.x * n;
    topv += (int64_t)blockIdx.x * k;
    topi += (int64_t)blockIdx.x * k;
    for (int it = 0; it < k; ++it) {
        double bv = NEG_INF;
        int64_t bi = IDX_NONE;
        int64_t bpos = -1;
        for (int64_t e = threadIdx.x; e < n; e += 256) {
            const int64_t idx = blki[e];
            if (idx != IDX_NONE && better(blkv[e], idx, bv, bi)) { bv = blkv[e]; bi = idx; bpos = e; }
        }
        const int64_t mine = bi;
        block_argmax(bv, bi, sv, si);
        if (bi != IDX_NONE && mine == bi && bpos >= 0) blki[bpos] = IDX_NONE;  // consume
        if (threadIdx.x == 0) { topv[it] = bv; topi[it] = (bi == IDX_NONE) ? -1 : bi; }
        __syncthreads();
    }
}

void launch_topk_merge(hipStream_t s, double* vals, int64_t* idx, int64_t n, int k, double* topv, int64_t* topi) {
    hipLaunchKernelGGL(k_topk_merge, dim3(1), dim3(256), 0, s, vals, idx, n, k, topv, topi);
}


// The k <= TOPK_PASS best of EACH of S value rows (row q at vals + q M) in two launches instead of 2 S (a Thompson sweep of
// 64 draws ranked its rows one after the other: 128 launches of 5 us).  blkv / blki: S * nblk * k entries; topv / topi: (S, k).
void launch_topk_rows(hipStream_t s, const double* vals, int64_t M, int64_t S, int k, double* blkv, int64_t* blki,
                      int64_t nblk, double* topv, int64_t* topi) {
    hipLaunchKernelGGL(k_topk_block, dim3((unsigned)nblk, (unsigned)S), dim3(256), 0, s, vals, M, k, blkv, blki,
                       (const double*)nullptr, (const int64_t*)nullptr);
    hipLaunchKernelGGL(k_topk_merge, dim3((unsigned)S), dim3(256), 0, s, blkv, blki, nblk * k, k, topv, topi);
}

// k <= TOPK_MAX entries, TOPK_PASS per pass: pass p ranks only what comes strictly after the last entry of pass p-1
// (value descending, index ascending: a total order, so the passes concatenate to exactly the k best).  blkv / blki need
// nblk * min(k, TOPK_PASS) entries; topv / topi k.  The reference's ranking is a full argsort (pybo/solvers/lbfgs.py:51).
void launch_topk(hipStream_t s, const double* vals, int64_t M, int k, double* blkv, int64_t* blki,
                 int64_t nblk, double* topv, int64_t* topi) {
    for (int done = 0; done < k; done += TOPK_PASS) {
        const int kk = (k - done < TOPK_PASS) ? k - done : TOPK_PASS;
        const double* cv = done ? topv + done - 1 : nullptr;
        const int64_t* ci = done ? topi + done - 1 : nullptr;
        hipLaunchKernelGGL(k_topk_block, dim3((unsigned)nblk), dim3(256), 0, s, vals, M, kk, blkv, blki, cv, ci);
        hipLaunchKernelGGL(k_topk_merge, dim3(1), dim3(256), 0, s, blkv, blki, nblk * kk, kk, topv + done, topi + done);
    }
}

// ------------------------------------------------------------------------------------------------
// Selection-only sweeps: a caller that asks for the k best candidates and for no per-candidate
// output needs the exact variance only of candidates that can reach the top-k.  EI is non-decreasing in the mean and in
// the standard deviation and s2 <= rho, so EI(mu + delta, sqrt(rho)) bounds a candidate's value from above at the cost of
// one row-dot with alpha (N covariance evaluations) instead of the N^2 flop of its column of V = T K*.
// ------------------------------------------------------------------------------------------------
constexpr double PRUNE_TAU_MIN = 1e-280;   // below this the k-th best seed value prunes nothing (relative error bounds need normal numbers)
constexpr double PRUNE_SLACK = 1e-6;       // relative rounding of acq_value(EI): <= 16 z^4 eps with z^2 <= 1500 wherever EI >= 1e-280, i.e. 4e-9

// alpha2_k = sum_m U[k][m] a_m (row k of U = R^-1 from its diagonal on) and sabs_k = sum_m |U[k][m] a_m|: the weights of the
// bound pass and the terms of S = || |T|^T |a| ||_1, from the very U and a the sweep kernel multiplies with (whatever
// fit / append sequence produced them).  One workgroup per row, fixed reduction tree.
__global__ __launch_bounds__(256) void k_prune_alpha(const double* __restrict__ U, int64_t Np, const double* __restrict__ a,
                                                     double* __restrict__ alpha2, double* __restrict__ sabs) {
    __shared__ double r0[256], r1[256];
    const int64_t k = blockIdx.x;
    const double* row = U + k * Np;
    double s = 0.0, t = 0.0;
    for (int64_t m = k + threadIdx.x; m < Np; m += 256) {
        const double pr = row[m] * a[m];
        s += pr;
        t += fabs(pr);
    }
    r0[threadIdx.x] = s;
    r1[threadIdx.x] = t;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            r0[threadIdx.x] += r0[threadIdx.x + w];
            r1[threadIdx.x] += r1[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        alpha2[k] = r0[0];
        sabs[k] = r1[0];
    }
}

// sc[0] = S, sc[1] = delta = 8 (Np + 16) 2^-53 (rho S + |bias|), sc[2..3] = {-1, 0}: the `pscal` that makes k_sweep_rankq
// return the plain dot product.  The bound of |mu_est - (bias + p)| is derived in DESIGN.md section 2.1.
__global__ __launch_bounds__(256) void k_prune_delta(const double* __restrict__ sabs, int64_t Np, double rho, double bias,
                                                     double* __restrict__ sc) {
    __shared__ double r0[256];
    double s = 0.0;
    for (int64_t m = threadIdx.x; m < Np; m += 256) s += sabs[m];
    r0[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) r0[threadIdx.x] += r0[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        sc[0] = r0[0];
        sc[1] = 8.0 * (double)(Np + 16) * 1.1102230246251565e-16 * fma(rho, r0[0], fabs(bias));   // (one rounding, whatever -ffp-contract says: gp_ref.prune_delta restates it)
        sc[2] = -1.0;
        sc[3] = 0.0;
    }
}

void launch_prune_alpha(hipStream_t s, const double* U, int64_t Np, const double* a, double rho, double bias, double* alpha2,
                        double* sabs, double* sc) {
    hipLaunchKernelGGL(k_prune_alpha, dim3((unsigned)Np), dim3(256), 0, s, U, Np, a, alpha2, sabs);
    hipLaunchKernelGGL(k_prune_delta, dim3(1), dim3(256), 0, s, sabs, Np, rho, bias, sc);
}

// ------------------------------------------------------------------------------------------------
// The bound pass's dot alpha2 . k(X, z_n) for the SE-ARD covariance with the distances on the matrix pipe.
// With x~, z~ the scaled coordinates minus a common centre c,  -r2 / 2 = x~ . z~ - |x~|^2 / 2 - |z~|^2 / 2  is ONE inner
// product of length d + 2: observation row [x~_1 .. x~_d, -|x~|^2 / 2, 1] times candidate column [z~_1 .. z~_d, 1, -|z~|^2 / 2],
// both padded with zeros to 4 KS.  v_mfma_f64_16x16x4_f64 forms it for 16 observations x 16 candidates in KS instructions
// while the VALU evaluates the exponentials of the tile before.  Where the two norm slots would cost an MFMA of their own
// (d mod 4 in {0, 3}) the inner product keeps its d terms and the norms arrive through the accumulator: it starts from
// (-|x~|^2 / 2) + (-|z~|^2 / 2), one addition per result instead of a quarter MFMA (64 cycles per 256 results).
// The exponential is bound_exp.h's table form: 18.3 VALU instructions per covariance in the walk's loop (19.2 with the addition)
// and one LDS read, where exp_nonpos made it 25.3; 46 in the generic kernel.
// The inner-product form cancels where the direct differences do not; sc[] carries the radii of the centred data and the
// guard k_bound_guard derives from them: sc[9] = 1.0 says this kernel runs, 0.0 says k_sweep_rankq<1> does (both read it).
// ------------------------------------------------------------------------------------------------
int bound_mfma_ks(int kernel_id, int d) { return (kernel_id == GPX_KERN_SE_ARD && d + 2 <= 4 * BM_KS_MAX) ? (d + 5) / 4 : 0; }

// the norms go through the accumulator where that saves an MFMA per tile; the k-steps of the kernel either way
static bool bound_mfma_normc(int d) { return d > 0 && (d + 3) / 4 < (d + 5) / 4; }
static int bound_mfma_steps(int d) { return bound_mfma_normc(d) ? (d + 3) / 4 : (d + 5) / 4; }

// max of non-negative doubles through their bit patterns (order-preserving for v >= 0); a NaN is not recorded
__device__ __forceinline__ void block_max_nonneg(double v, double* slot, double* red) {
    red[threadIdx.x] = (v == v) ? v : 0.0;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0)
        atomicMax(reinterpret_cast<unsigned long long*>(slot), (unsigned long long)__double_as_longlong(red[0]));
}

// cen[k] = midpoint of the scaled observations' box in dimension k; clears the two radius slots.  One workgroup.
__global__ __launch_bounds__(256) void k_bound_centre(const double* __restrict__ Xs, int64_t N, int d, double* __restrict__ cen,
                                                      double* __restrict__ sc) {
    __shared__ double lo[256], hi[256];
    for (int k = 0; k < d; ++k) {
        double a = __builtin_huge_val(), b = -__builtin_huge_val();
        for (int64_t i = threadIdx.x; i < N; i += 256) {
            const double x = Xs[i * d + k];
            a = fmin(a, x);
            b = fmax(b, x);
        }
        lo[threadIdx.x] = a;
        hi[threadIdx.x] = b;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) {
                lo[threadIdx.x] = fmin(lo[threadIdx.x], lo[threadIdx.x + w]);
                hi[threadIdx.x] = fmax(hi[threadIdx.x], hi[threadIdx.x + w]);
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) cen[k] = 0.5 * lo[0] + 0.5 * hi[0];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        sc[BM_SC_RX2] = 0.0;
        sc[BM_SC_RZ2] = 0.0;
        sc[BM_SC_BADW] = 0.0;
    }
}

// The augmented observation array in fragment order: tile t (16 rows), k-step ks, lane l holds element k = 4 ks + (l >> 4) of row
// 16 t + (l & 15) at A[(t KS + ks) 64 + l] -- one coalesced 512-byte read per wave and k-step.  W4[16 t + 4 g + r] = rho alpha2 of row
// 16 t + g + 4 r: the four weights of a lane's four results (C/D row = (l >> 4) + 4 r) as one 32-byte read.  Rows from N on: zeros.
// NX4 (non-null: the norms go through the accumulator): -|x~|^2 / 2 in W4's order, and the rows are [x~_1 .. x~_d] alone.
// A32 (non-null: the fp32 link may run): the same three arrays once more in fp32, Np + 16 rows in the sign-homogeneous order of
// bound_f32.h (w > 0, 16 zero rows, w == 0, w < 0; sc[TPOS32] = the first tile without a positive weight): the coordinates at A32, behind
// them the weights, the factorised walk's weights w r_i and, with NX4, the norms, Np + 16 floats each -- the coordinates and the norm
// times log2(e), each rounded once from the fp64 value; weights and norms in row order -- and sc[BADW] = 1.0 where a weight is neither 0
// nor a normal fp32 number, 0.5 where only a weight of the factorised walk is not.
__global__ __launch_bounds__(256) void k_bound_aug(const double* __restrict__ Xs, int64_t N, int64_t Np, int d, int KS,
                                                   const double* __restrict__ cen, const double* __restrict__ alpha2, double rho,
                                                   double* __restrict__ A, double* __restrict__ W4, double* __restrict__ NX4,
                                                   float* __restrict__ A32, double* __restrict__ sc) {
    __shared__ double red[256];
    __shared__ int cnt[4], wcnt[4][2];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;       // (Np is a multiple of 128)
    // The fp32 copies' row of row i (bound_f32.h, sign-homogeneous tiles): every workgroup counts the signs of all weights, and of those
    // before its own rows, itself (Np / 256 weights a thread) -- no launch and no pass of their own; ranks inside the workgroup by ballot.
    int64_t i32 = 0, npos = 0;
    if (A32) {
        if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
        __syncthreads();
        const int64_t i0 = (int64_t)blockIdx.x * 256;
        int c[4] = {0, 0, 0, 0};      // w > 0 and w == 0 (not < 0, not > 0) among all rows / among the rows before this workgroup's
        for (int64_t j = threadIdx.x; j < Np; j += 256) {
            const double wj = (j < N) ? rho * alpha2[j] : 0.0;
            const int p = wj > 0.0 ? 1 : 0, z = (wj > 0.0 || wj < 0.0) ? 0 : 1;
            c[0] += p;
            c[1] += z;
            c[2] += (j < i0) ? p : 0;
            c[3] += (j < i0) ? z : 0;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            for (int o = 32; o > 0; o >>= 1) c[q] += __shfl_xor(c[q], o);
            if ((threadIdx.x & 63) == 0) atomicAdd(&cnt[q], c[q]);
        }
        const double wi = (i < N) ? rho * alpha2[i] : 0.0;
        const bool in = i < Np, p = in && wi > 0.0, z = in && !(wi > 0.0 || wi < 0.0);
        const unsigned long long bp = __ballot(p), bz = __ballot(z), below = (1ull << (threadIdx.x & 63)) - 1ull;
        const int wv = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) {
            wcnt[wv][0] = __popcll(bp);
            wcnt[wv][1] = __popcll(bz);
        }
        __syncthreads();
        int rp = cnt[2] + __popcll(bp & below), rz = cnt[3] + __popcll(bz & below);
        for (int q = 0; q < wv; ++q) {
            rp += wcnt[q][0];
            rz += wcnt[q][1];
        }
        npos = cnt[0];
        const int64_t rn = i - rp - rz;                               // the rows before i that are neither: w < 0
        i32 = bound32_row_dest(p ? 1 : (z ? 0 : -1), p ? rp : (z ? rz : rn), npos, cnt[1]);
        if (i == 0) sc[BM_SC_TPOS32] = (double)bound32_tpos(npos);
    }
    double n2 = 0.0, badw = 0.0;
    if (i < Np) {
        const int64_t t = i >> 4, t32 = i32 >> 4;
        const int row = (int)(i & 15), row32 = (int)(i32 & 15);
        double* At = A + t * KS * 64 + row;
        const bool live = i < N;
        for (int k = 0; k < 4 * KS; ++k) {
            double v = 0.0;
            if (live && k < d) {
                v = Xs[i * d + k] - cen[k];
                n2 = fma(v, v, n2);
            }
            if (live && !NX4 && k == d) v = -0.5 * n2;
            if (live && !NX4 && k == d + 1) v = 1.0;
            At[(k >> 2) * 64 + (k & 3) * 16] = v;
            if (A32) A32[t32 * KS * 64 + row32 + (k >> 2) * 64 + (k & 3) * 16] = (float)((live && k <= d) ? B32_LOG2E * v : v);
        }
        const int g = row & 3, r = row >> 2;                          // row = g + 4 r
        const double wt = live ? rho * alpha2[i] : 0.0;
        W4[t * 16 + 4 * g + r] = wt;
        if (NX4) NX4[t * 16 + 4 * g + r] = live ? -0.5 * n2 : 0.0;
        if (A32) {
            const int64_t Np32 = Np + B32_ZROWS;
            float* W32 = A32 + Np32 * 4 * KS;
            const double wf = wt * bound32_norm_factor(n2);           // the factorised walk's weight: the row's norm factor goes in before the one rounding
            W32[i32] = (float)wt;    // (row order: the fp32 MFMA's C/D row is 4 (l >> 4) + r, a lane's four results are four neighbouring rows)
            W32[Np32 + i32] = (float)wf;
            if (NX4) W32[2 * Np32 + i32] = live ? (float)(B32_LOG2E * (-0.5 * n2)) : 0.0f;
            badw = fmax(bound32_bad_weight(wt), 0.5 * bound32_bad_weight_fact(wt, wf));
            if (i < B32_ZROWS) {                                      // the extra zero tile's rows, behind the positive weights
                const int64_t e = npos + i;
                for (int k = 0; k < 4 * KS; ++k) A32[(e >> 4) * KS * 64 + (e & 15) + (k >> 2) * 64 + (k & 3) * 16] = 0.0f;
                W32[e] = W32[Np32 + e] = 0.0f;
                if (NX4) W32[2 * Np32 + e] = 0.0f;
            }
        }
    }
    block_max_nonneg(n2, sc + BM_SC_RX2, red);
    if (A32) block_max_nonneg(badw, sc + BM_SC_BADW, red);
}

// sc[RZ2] = max_n |z~_n|^2 over the candidates (NaN rows are not recorded: their bound is NaN whatever the kernel; an infinite
// coordinate makes the radius infinite and the guard decline)
__global__ __launch_bounds__(256) void k_bound_rz(const double* __restrict__ Z, int64_t M, int d, const double* __restrict__ invell,
                                                  const double* __restrict__ cen, double* __restrict__ sc) {
    __shared__ double red[256];
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double n2 = 0.0;
    if (n < M)
        for (int k = 0; k < d; ++k) {
            const double v = bound_zt(Z[n * d + k], invell[k], cen[k]);
            n2 = fma(v, v, n2);
        }
    block_max_nonneg(n2, sc + BM_SC_RZ2, red);
}

// The guard: the inner-product form's exponent errs by at most (d + 4) u (R_x + R_z)^2, which the margin
// delta / 2 has room for while that is at most Np u.  force: -1 by guard, 1 the matrix-pipe kernel whatever the guard says.
// The fp32 link (want32: its operands exist and the host's size rule allows it; force 2: whatever the guards say) runs where the fp64
// guard passes, E <= 2^-10 and every weight is 0 or a normal fp32 number; sc[E32] is NaN where it was not considered.
// The factorised walk (allow_fact: option bound_fact) runs where the fp32 kernel does, its own guards hold whatever `force` says, and
// bound32_fact_ok passes the radii and the weights' sum with no scaled weight outside fp32's normal range.
__global__ void k_bound_guard(int d, int64_t Np, int force, int want32, int allow_fact, double rho, double* __restrict__ sc) {
    const double R = sqrt(sc[BM_SC_RX2]) + sqrt(sc[BM_SC_RZ2]);
    const double gv = (double)(d + 4) * R * R;
    const bool use64 = force > 0 || gv <= (double)Np;
    sc[BM_SC_GUARD] = gv;
    sc[BM_SC_USE] = use64 ? 1.0 : 0.0;
    double E = __builtin_nan(""), use32 = 0.0, fact = 0.0, fac = 0.0, fl = 0.0;
    if (want32) {
        const double bw = sc[BM_SC_BADW], sum_w = rho * sc[0] * (1.0 + 0x1p-20);
        E = bound32_E(d, (double)(Np / 16), gv);
        use32 = (force == 2 || (use64 && E <= B32_E_MAX && bw != 1.0)) ? 1.0 : 0.0;
        fact = (allow_fact && use32 == 1.0 && E <= B32_E_MAX && bw == 0.0) ? bound32_fact_ok(sc[BM_SC_RX2], sc[BM_SC_RZ2], sum_w) : 0.0;
        fac = bound32_factor(E, bw == 1.0 ? 1.0 : 0.0);
        fl = bound32_flush(sum_w, (double)Np);
    }
    sc[BM_SC_E32] = E;
    sc[BM_SC_USE32] = use32;
    sc[BM_SC_FAC32] = fac;
    sc[BM_SC_FACT32] = fact;
    sc[BM_SC_FLUSH32] = fl;
}

// One workgroup owns 128 candidates (8 column tiles of 16, their fragments in registers for the whole walk); wave w walks the
// 16-row tiles w, w + 4, .. of the augmented array in order.  Per tile and column tile: KS MFMAs from a zero accumulator (NC: from
// the sum of the two norms), then per result the exponent limited to <= 0, bound_exp from the table in LDS, one FMA with the row's
// weight into the lane's accumulator of that column.  The two limits are v_min_f64 / v_max_f64, which drop a NaN: a candidate whose
// |z~|^2 is not finite (a NaN or infinite coordinate, an overflow) gets its NaN back once, after the walk.  The four row groups of a
// wave are combined by two exchanges, the waves through LDS, in a fixed order: the values do not depend on the launch geometry.
template <int KS, bool NC>
__global__ __launch_bounds__(256, (KS + (NC ? 1 : 0) <= 3) ? 4 : 3) void k_bound_mfma(const double* __restrict__ A, const double* __restrict__ W4,
                                                       const double* __restrict__ NX4, int ntile, int d, const double* __restrict__ Z,
                                                       int64_t M, const double* __restrict__ invell, const double* __restrict__ cen,
                                                       const double* __restrict__ sc, double* __restrict__ out) {
    __shared__ double red[4][XN];
    __shared__ double tab[BEXP_NT];
    if (sc[BM_SC_USE] != 1.0 || sc[BM_SC_USE32] == 1.0) return;
    if (threadIdx.x < BEXP_NT) tab[threadIdx.x] = kBoundExpTab[threadIdx.x];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // (w in a scalar register: the walk's loop is uniform)
    const int col = lane & 15, g = lane >> 4;
    const int64_t n0 = (int64_t)blockIdx.x * XN;
    double b[8][KS], nz[NC ? 8 : 1];
    unsigned lost = 0;                        // bit j: column tile j's candidate has no finite |z~|^2
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int64_t n = n0 + j * 16 + col;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) b[j][ks] = 0.0;
        double n2 = 0.0;
        if (n < M) {
            for (int k = 0; k < d; ++k) {
                const double v = bound_zt(Z[n * d + k], invell[k], cen[k]);
                n2 = fma(v, v, n2);
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) b[j][ks] = (k == 4 * ks + g) ? v : b[j][ks];
            }
            if (!NC) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    b[j][ks] = (d == 4 * ks + g) ? 1.0 : b[j][ks];
                    b[j][ks] = (d + 1 == 4 * ks + g) ? -0.5 * n2 : b[j][ks];
                }
            }
        }
        if (NC) nz[j] = -0.5 * n2;
        lost |= (n2 < __builtin_huge_val()) ? 0u : (1u << j);
    }
    __syncthreads();
    double acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.0;
    // byte offsets in 32 bits from the kernel's (scalar) pointers: one register each where a pointer takes two (A: 32 KS Np bytes)
    unsigned ao = ((unsigned)w * KS * 64 + lane) * 8, wo = ((unsigned)w * 16 + g * 4) * 8, xo = wo;
    const auto ld1 = [](const double* p, unsigned o) { return *reinterpret_cast<const double*>(reinterpret_cast<const char*>(p) + o); };
    const auto ld4 = [](const double* p, unsigned o) { return *reinterpret_cast<const d4*>(reinterpret_cast<const char*>(p) + o); };
    double a[KS], an[KS];
    d4 wv, wn = {0.0, 0.0, 0.0, 0.0}, xv = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) an[ks] = ld1(A, ao + ks * 512);
    if (NC)
        xv = ld4(NX4, xo);
    else
        wn = ld4(W4, wo);
#pragma unroll 1
    for (int t = w; t < ntile; t += 4) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) a[ks] = an[ks];
        // NC keeps 8 norms where the other form keeps 8 more fragments, and the row norms besides: no second buffer for either vector.
        // The weights are first wanted a whole exponential into the tile, the norms (below) are read behind their last use.
        wv = NC ? ld4(W4, wo) : wn;
        wo += 4 * 16 * 8;
        if (t + 4 < ntile) {                  // the next tile's operands while this one computes
            ao += 4 * KS * 64 * 8;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) an[ks] = ld1(A, ao + ks * 512);
            if (!NC) wn = ld4(W4, wo);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            d4 c = {0.0, 0.0, 0.0, 0.0};
            if (NC) {
#pragma unroll
                for (int r = 0; r < 4; ++r) c[r] = xv[r] + nz[j];
                if (j == 7) {                 // the last use of this tile's norms: the next tile's take their place
                    xo += (t + 4 < ntile) ? 4 * 16 * 8 : 0;
                    xv = ld4(NX4, xo);
                }
            }
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) c = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], b[j][ks], c, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[j] = fma(wv[r], bound_exp<false>(__builtin_fmin(c[r], 0.0), tab), acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        double v = acc[j];
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        if (g == 0) red[w][j * 16 + col] = ((lost >> j) & 1u) ? __builtin_nan("") : v;
    }
    __syncthreads();
    if (threadIdx.x < XN) {
        const int64_t n = n0 + threadIdx.x;
        if (n < M) out[n] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    }
}

// Prologue, guard and the matrix-pipe kernels on stream s.  ws: the operands' block (bound_ops); sc: the bound pass's BM_SC_WORDS scalars.
// force: the option prune_bound (-1, 1, 2); allow32: the host's size rule lets the fp32 link run by its guards; allow_fact: option bound_fact.
// The caller launches the generic kernel behind it with sc + BM_SC_USE as its `skip`: exactly one of the three writes `out`.
void launch_bound_mfma(hipStream_t s, const double* Xs, int64_t N, int64_t Np, int d, const double* alpha2, double rho,
                       const double* Z, int64_t M, const double* invell, int force, bool allow32, bool allow_fact, double* ws, double* sc,
                       double* out) {
    const int KS = bound_mfma_steps(d);
    const bool nc = bound_mfma_normc(d);
    WsCarver c(ws);
    const BoundOps o = bound_ops(c, Np, KS, nc);
    const bool want32 = force == 2 || (force < 0 && allow32);
    const int64_t Np32 = Np + B32_ZROWS;
    float* const A32 = want32 ? o.A32 : nullptr;
    const float *const W32 = want32 ? o.W32 : nullptr, *const WF32 = want32 ? o.WF32 : nullptr, *const NX32 = want32 ? o.NX32 : nullptr;
    hipLaunchKernelGGL(k_bound_centre, dim3(1), dim3(256), 0, s, Xs, N, d, o.cen, sc);
    hipLaunchKernelGGL(k_bound_aug, dim3((unsigned)((Np + 255) / 256)), dim3(256), 0, s, Xs, N, Np, d, KS, o.cen, alpha2, rho, o.A, o.W4, o.NX4, A32, sc);
    hipLaunchKernelGGL(k_bound_rz, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, Z, M, d, invell, o.cen, sc);
    hipLaunchKernelGGL(k_bound_guard, dim3(1), dim3(1), 0, s, d, Np, force, want32 ? 1 : 0, allow_fact ? 1 : 0, rho, sc);
    const dim3 grid((unsigned)((M + XN - 1) / XN));
    const int ntile = (int)(Np / 16);
#define GPX_BM(K, C) hipLaunchKernelGGL((k_bound_mfma<K, C>), grid, dim3(256), 0, s, o.A, o.W4, o.NX4, ntile, d, Z, M, invell, o.cen, sc, out)
    switch (2 * KS + (nc ? 1 : 0)) {
        case 2: GPX_BM(1, false); break;
        case 3: GPX_BM(1, true); break;
        case 4: GPX_BM(2, false); break;
        case 5: GPX_BM(2, true); break;
        case 6: GPX_BM(3, false); break;
        case 7: GPX_BM(3, true); break;
        case 8: GPX_BM(4, false); break;
        case 9: GPX_BM(4, true); break;
        default: GPX_BM(5, false); break;
    }
#undef GPX_BM
    if (!want32) return;
    launch_bound_mfma32(s, A32, W32, WF32, NX32, KS, nc, (int)(Np32 / 16), d, Z, M, invell, o.cen, sc, out);
}

// ub[n] <- EI((bias + dots[n]) + delta, s2 = rho), dots[n] = alpha2 . k(X, z_n) (ei_mean_bound, gpx_math.h); -inf for the `skip`
// leading candidates that are exactly evaluated already.  The dots stay where they are: the second bound reads them again.
__global__ __launch_bounds__(256) void k_prune_ub(const double* __restrict__ dots, double* __restrict__ ub, int64_t M, int64_t skip,
                                                  const double* __restrict__ sc, double rho, double bias, double p0) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= M) return;
    ub[n] = (n < skip) ? NEG_INF : ei_mean_bound(bias, dots[n], sc[1], rho, p0);
}

void launch_prune_ub(hipStream_t s, const double* dots, double* ub, int64_t M, int64_t skip, const double* sc, double rho,
                     double bias, double p0) {
    hipLaunchKernelGGL(k_prune_ub, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, dots, ub, M, skip, sc, rho, bias, p0);
}

// The second bound of a selection-only sweep, for survivor j of the chunk at j0: qR = the sum of the
// row-prefix launch's Qp[rb][j], rb < nR, by the loop k_acq sums its q with (add_rowblocks) -- every term a sum of squares, so no
// larger than k_acq's q, bit for bit -- s2R = s2_floored(rho, qR) >= s2 and ub2 = EI((bias + dot) + delta, s2R) with k_prune_ub's mean bound.
// qR_out (optional) keeps the sums for gpx_prune_rows.
__global__ __launch_bounds__(256) void k_prune_ub2(const double* __restrict__ Qp, int64_t ldp, int nR, int64_t j0, int64_t cols_valid,
                                                   const int64_t* __restrict__ idx, const double* __restrict__ dots,
                                                   const double* __restrict__ sc, double rho, double bias, double p0,
                                                   double* __restrict__ ub2, double* __restrict__ qR_out) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= cols_valid) return;
    double q = 0.0, unused = 0.0;
    add_rowblocks<false>(Qp, nullptr, ldp, nR, n, q, unused);
    ub2[j0 + n] = ei_mean_bound(bias, dots[idx[j0 + n]], sc[1], s2_floored(rho, q), p0);
    if (qR_out) qR_out[j0 + n] = q;
}

void launch_prune_ub2(hipStream_t s, const double* Qp, int64_t ldp, int nR, int64_t j0, int64_t cols_valid, const int64_t* idx,
                      const double* dots, const double* sc, double rho, double bias, double p0, double* ub2, double* qR_out) {
    hipLaunchKernelGGL(k_prune_ub2, dim3((unsigned)((cols_valid + 255) / 256)), dim3(256), 0, s, Qp, ldp, nR, j0, cols_valid, idx,
                       dots, sc, rho, bias, p0, ub2, qR_out);
}

// idx2[j] <- idx[idx2[j]]: the second cut compacts positions of the first-level list; these are the candidates behind them
__global__ __launch_bounds__(256) void k_sel_remap(const int64_t* __restrict__ idx, int64_t* __restrict__ idx2, int64_t n) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < n) idx2[j] = idx[idx2[j]];
}

void launch_sel_remap(hipStream_t s, const int64_t* idx, int64_t* idx2, int64_t n) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_sel_remap, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, idx, idx2, n);
}

// The ensemble's bound.  The sum of the members' bounds and its division are k_ens_accum's and k_ens_finish's own
// (ens_fold in mode 0, ens_mean: acq_core.h): one addition per member in member order, one division -- never contracted with
// the last multiply of acq_value -- so that ub_m >= v_m for every member gives a result >= the exact chain's, bit for bit.

// acc[c] (+)= EI((bias + dots[c]) + delta, s2 = rho): k_prune_ub's value of one member, folded into the running sum in the same
// pass; delta_out receives the member's delta = sc[1] and fact_out 1.0 where its dots came from the fp32 kernel's factorised walk (guarded:
// the device chose the kernel; NaN otherwise) (for gpx_ensemble_prune_report).
__global__ __launch_bounds__(256) void k_prune_ub_fold(const double* __restrict__ dots, double* __restrict__ acc, int64_t M,
                                                       const double* __restrict__ sc, double rho, double bias, double p0, int first,
                                                       double* __restrict__ delta_out, int guarded, double* __restrict__ fact_out) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= M) return;
    double a0 = first ? 0.0 : acc[n], unused = 0.0;
    ens_fold(0, first, ei_mean_bound(bias, dots[n], sc[1], rho, p0), 0.0, a0, unused);
    acc[n] = a0;
    if (n == 0) {
        *delta_out = sc[1];
        *fact_out = guarded ? ((sc[BM_SC_USE32] == 1.0 && sc[BM_SC_FACT32] == 1.0) ? 1.0 : 0.0) : __builtin_nan("");
    }
}

void launch_prune_ub_fold(hipStream_t s, const double* dots, double* acc, int64_t M, const double* sc, double rho, double bias,
                          double p0, int first, double* delta_out, int guarded, double* fact_out) {
    hipLaunchKernelGGL(k_prune_ub_fold, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, dots, acc, M, sc, rho, bias, p0, first,
                       delta_out, guarded, fact_out);
}

// acc[c] <- acc[c] / n, the ensemble's bound; -inf for the `skip` leading candidates that are exactly evaluated already
__global__ __launch_bounds__(256) void k_prune_ub_mean(double* __restrict__ acc, int64_t M, int64_t skip, double n) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= M) return;
    acc[c] = (c < skip) ? NEG_INF : ens_mean(acc[c], n);
}

void launch_prune_ub_mean(hipStream_t s, double* acc, int64_t M, int64_t skip, double n) {
    hipLaunchKernelGGL(k_prune_ub_mean, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, acc, M, skip, n);
}

// out[0] = mean of v[0..n)  (the gate of a selection-only sweep: the mean s2 of its first generation)
__global__ __launch_bounds__(256) void k_prune_mean(const double* __restrict__ v, int64_t n, double* __restrict__ out) {
    __shared__ double r0[256];
    double s = 0.0;
    for (int64_t m = threadIdx.x; m < n; m += 256) s += v[m];
    r0[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) r0[threadIdx.x] += r0[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = r0[0] / (double)n;
}

void launch_prune_mean(hipStream_t s, const double* v, int64_t n, double* out) {
    hipLaunchKernelGGL(k_prune_mean, dim3(1), dim3(256), 0, s, v, n, out);
}

// Order-preserving 24-bit key of a double (sign, exponent, 12 mantissa bits): a <= b implies key(a) <= key(b).
__device__ __forceinline__ unsigned sel_key24(double v) {
    unsigned long long b = (unsigned long long)__double_as_longlong(v);
    b ^= (b >> 63) ? ~0ull : 0x8000000000000000ull;
    return (unsigned)(b >> 40);
}

// Radix select of the G-th largest key in two passes of 12 bits.  st: [0] bin of pass 0, [1] elements in higher bins,
// [2] the threshold key: at least G elements have key >= st[2].
__global__ __launch_bounds__(256) void k_sel_hist(const double* __restrict__ v, int64_t M, int pass, const int* __restrict__ st,
                                                  int* __restrict__ hist) {
    __shared__ int lh[SEL_BINS];
    for (int b = threadIdx.x; b < SEL_BINS; b += 256) lh[b] = 0;
    __syncthreads();
    const unsigned hi = pass ? (unsigned)st[0] : 0u;
    const int64_t base = (int64_t)blockIdx.x * SEL_PER_BLOCK;
    for (int e = 0; e < SEL_PER_THREAD; ++e) {
        const int64_t n = base + e * 256 + threadIdx.x;
        if (n >= M) break;
        const unsigned key = sel_key24(v[n]);
        if (!pass) atomicAdd(&lh[key >> 12], 1);
        else if ((key >> 12) == hi) atomicAdd(&lh[key & 4095u], 1);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < SEL_BINS; b += 256)
        if (lh[b]) atomicAdd(&hist[b], lh[b]);
}

__global__ __launch_bounds__(256) void k_sel_pick(const int* __restrict__ hist, int pass, int G, int* __restrict__ st) {
    __shared__ int ts[256];
    int s = 0;
    for (int j = 0; j < 16; ++j) s += hist[threadIdx.x * 16 + j];
    ts[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int need = pass ? G - st[1] : G;
        int cum = 0, t = 255;
        for (; t > 0; --t) {
            if (cum + ts[t] >= need) break;
            cum += ts[t];
        }
        int b = t * 16 + 15;
        for (; b > t * 16; --b) {
            if (cum + hist[b] >= need) break;
            cum += hist[b];
        }
        if (!pass) {
            st[0] = b;
            st[1] = cum;
        } else {
            st[2] = (st[0] << 12) | b;
        }
    }
}

void launch_sel_threshold(hipStream_t s, const double* v, int64_t M, int G, int* hist, int* st) {
    const unsigned nblk = (unsigned)((M + SEL_PER_BLOCK - 1) / SEL_PER_BLOCK);
    (void)hipMemsetAsync(hist, 0, 2 * SEL_BINS * sizeof(int), s);
    for (int pass = 0; pass < 2; ++pass) {
        hipLaunchKernelGGL(k_sel_hist, dim3(nblk), dim3(256), 0, s, v, M, pass, st, hist + pass * SEL_BINS);
        hipLaunchKernelGGL(k_sel_pick, dim3(1), dim3(256), 0, s, hist + pass * SEL_BINS, pass, G, st);
    }
}

// Stable compaction.  mode 0 (seeds): the `cap` = G first candidates in (key descending, index ascending) order -- every
// key above the threshold st[2] (class A: fewer than G by the threshold's definition) and, of the keys equal to it (class E),
// the first G - |A| by index.  mode 1 (survivors): NOT v < tau (1 - slack), so a NaN bound survives and an evaluated
// candidate (v = -inf) does not; a tau that is not a normal positive number prunes nothing (all of class E, none of A).
// A block's two counts travel as one word, E + (A << 40), through the same scan (|A| < 2^23, |E| <= M < 2^40).
constexpr int SEL_A_SHIFT = 40;
constexpr long long SEL_E_MASK = (1ll << SEL_A_SHIFT) - 1;
__device__ __forceinline__ long long sel_class(int mode, double v, unsigned thr, double cut) {
    if (mode == 0) {
        const unsigned key = sel_key24(v);
        return key > thr ? (1ll << SEL_A_SHIFT) : (key == thr ? 1ll : 0ll);
    }
    return !(v < cut) ? 1ll : 0ll;
}
__device__ __forceinline__ double sel_cut(int mode, const double* tau) {
    if (mode == 0) return 0.0;
    const double t = *tau;
    return (t >= PRUNE_TAU_MIN) ? t * (1.0 - PRUNE_SLACK) : NEG_INF;
}

__global__ __launch_bounds__(256) void k_sel_count(const double* __restrict__ v, int64_t M, int mode, const int* __restrict__ st,
                                                   const double* __restrict__ tau, int64_t* __restrict__ blk,
                                                   double* __restrict__ tau_seen) {
    __shared__ unsigned long long cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    const unsigned thr = (unsigned)st[2];
    const double cut = sel_cut(mode, tau);
    const int64_t base = (int64_t)blockIdx.x * SEL_PER_BLOCK + (int64_t)threadIdx.x * SEL_PER_THREAD;
    long long c = 0;
    for (int e = 0; e < SEL_PER_THREAD; ++e)
        if (base + e < M) c += sel_class(mode, v[base + e], thr, cut);
    if (c) atomicAdd(&cnt, (unsigned long long)c);
    __syncthreads();
    if (threadIdx.x == 0) {
        blk[blockIdx.x] = (int64_t)cnt;
        if (tau_seen && blockIdx.x == 0) *tau_seen = *tau;      // the cut's tau, for gpx_prune_report (the top-k reuses its slot)
    }
}

// blk[0..nblk) counts -> exclusive offsets in place, blk[nblk] = total (one workgroup walks the blocks 256 at a time)
__global__ __launch_bounds__(256) void k_sel_scan(int64_t* __restrict__ blk, int64_t nblk) {
    __shared__ int64_t sh[256];
    __shared__ int64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int64_t b0 = 0; b0 < nblk; b0 += 256) {
        const int64_t i = b0 + threadIdx.x;
        const int64_t mine = (i < nblk) ? blk[i] : 0;
        sh[threadIdx.x] = mine;
        __syncthreads();
        for (int w = 1; w < 256; w <<= 1) {
            const int64_t add = ((int)threadIdx.x >= w) ? sh[threadIdx.x - w] : 0;
            __syncthreads();
            sh[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < nblk) blk[i] = carry + sh[threadIdx.x] - mine;
        __syncthreads();
        if (threadIdx.x == 255) carry += sh[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) blk[nblk] = carry;
}

// the selected candidates in their original order: idx[j] = n and row j of Xg = row n of Xc, for the first `cap` of them
__global__ __launch_bounds__(256) void k_sel_write(const double* __restrict__ v, int64_t M, int mode, const int* __restrict__ st,
                                                   const double* __restrict__ tau, const int64_t* __restrict__ blk, int64_t nblk,
                                                   int64_t cap, const double* __restrict__ Xc, int d, int64_t* __restrict__ idx,
                                                   double* __restrict__ Xg) {
    __shared__ long long sh[256];
    const unsigned thr = (unsigned)st[2];
    const double cut = sel_cut(mode, tau);
    // of class E, the first `need` by index are taken: all of them for the survivors, what the class A leaves of cap for the seeds
    const long long need = mode == 0 ? cap - (blk[nblk] >> SEL_A_SHIFT) : INT64_MAX;
    const int64_t base = (int64_t)blockIdx.x * SEL_PER_BLOCK + (int64_t)threadIdx.x * SEL_PER_THREAD;
    long long cls[SEL_PER_THREAD];
    long long mine = 0;
#pragma unroll
    for (int e = 0; e < SEL_PER_THREAD; ++e) {
        cls[e] = (base + e < M) ? sel_class(mode, v[base + e], thr, cut) : 0ll;
        mine += cls[e];
    }
    sh[threadIdx.x] = mine;
    __syncthreads();
    for (int w = 1; w < 256; w <<= 1) {
        const long long add = ((int)threadIdx.x >= w) ? sh[threadIdx.x - w] : 0;
        __syncthreads();
        sh[threadIdx.x] += add;
        __syncthreads();
    }
    long long before = blk[blockIdx.x] + sh[threadIdx.x] - mine;      // the two classes' counts ahead of this thread's first element
#pragma unroll
    for (int e = 0; e < SEL_PER_THREAD; ++e) {
        const long long c = cls[e];
        if (c) {
            const long long nA = before >> SEL_A_SHIFT, nE = before & SEL_E_MASK;
            const bool take = (c >> SEL_A_SHIFT) || nE < need;
            const long long off = nA + (nE < need ? nE : need);
            if (take && off < cap) {
                idx[off] = base + e;
                for (int q = 0; q < d; ++q) Xg[off * d + q] = Xc[(base + e) * d + q];
            }
            before += c;
        }
    }
}


// count only (total -> blk[nblk]) and the offsets the write needs.  tau_seen (optional): the survivor pass leaves the tau it cut
// with there -- one store by one thread, read only by gpx_prune_report; the shipping path carries it so that the diagnostic adds no
// launch and no copy to a sweep.
void launch_sel_compact(hipStream_t s, const double* v, int64_t M, int mode, const int* st, const double* tau, int64_t* blk,
                        int64_t cap, const double* Xc, int d, int64_t* idx, double* Xg, double* tau_seen) {
    const int64_t nblk = sel_blocks(M);
    hipLaunchKernelGGL(k_sel_count, dim3((unsigned)nblk), dim3(256), 0, s, v, M, mode, st, tau, blk, tau_seen);
    hipLaunchKernelGGL(k_sel_scan, dim3(1), dim3(256), 0, s, blk, nblk);
    hipLaunchKernelGGL(k_sel_write, dim3((unsigned)nblk), dim3(256), 0, s, v, M, mode, st, tau, blk, nblk, cap, Xc, d, idx, Xg);
}

// out[idx[j]] = vals[j] for j < n; mark (optional): those candidates' bounds -> -inf (evaluated: never a survivor)
__global__ __launch_bounds__(256) void k_sel_scatter(const int64_t* __restrict__ idx, const double* __restrict__ vals, int64_t n,
                                                     double* __restrict__ out, double* __restrict__ mark) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int64_t i = idx[j];
    out[i] = vals[j];
    if (mark) mark[i] = NEG_INF;
}

void launch_sel_scatter(hipStream_t s, const int64_t* idx, const double* vals, int64_t n, double* out, double* mark) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_sel_scatter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, idx, vals, n, out, mark);
}

__global__ __launch_bounds__(256) void k_fill_neg_inf(double* __restrict__ out, int64_t from, int64_t M) {
    const int64_t n = from + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n < M) out[n] = NEG_INF;
}

void launch_fill_neg_inf(hipStream_t s, double* out, int64_t from, int64_t M) {
    if (from >= M) return;
    hipLaunchKernelGGL(k_fill_neg_inf, dim3((unsigned)((M - from + 255) / 256)), dim3(256), 0, s, out, from, M);
}

}  // namespace gpx
