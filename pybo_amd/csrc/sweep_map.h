// sweep_map.h -- block -> tile maps of the dominant sweep kernel (kernels_sweep.hip: sweep_tiles) and the grid of a launch.
// Plain C++ without HIP types: the device code and the host launch share it, and tests/c/sweep_map_check.cpp compiles it into a
// host-only program that walks every grid and proves each map total and exact before a launch relies on it.
//
// A map turns a block index b into a tile (mt, nt) of the nR x NT tiles of a launch (mt: 128 observed rows, nt: 128 candidates) and,
// in the paired maps, a second tile (mt2, nt) the workgroup computes afterwards.  A tile's bits do not depend on the block that
// computes it (sweep_tiles), so every map gives the same result; maps differ in what the workgroups resident on one XCD share.
#ifndef GPX_SWEEP_MAP_H
#define GPX_SWEEP_MAP_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GPX_MAP_FN __host__ __device__ __forceinline__
#else
#define GPX_MAP_FN inline
#endif

namespace gpx {

// Orders 0 .. 3 are bits 0-1 of the option tile_order.  The short forms of order 3 are chosen by launch_sweep_trmm, never by a caller.
constexpr int SWEEP_ORDER_SHORT = 4;           // short form of order 3, pair rows of an XCD contiguous
constexpr int SWEEP_ORDER_SHORT_STRIDED = 5;   // the same with pair rows dealt round-robin over the m-groups (A/B and witness)

// Order 3 gives every XCD a slice of ceil(NT / 8) candidate tiles and ALL pair rows.  A launch whose slices are narrower than a
// super-tile (fewer than SN = RES / sm tiles) cannot fill the sm x SN patches: at NT = 16 every XCD holds 32 pair rows x 2 tiles,
// streams the whole factor and uses each row panel twice.  The short form splits the pair rows over the XCDs as well.
template <int RES>
GPX_MAP_FN bool sweep_map_is_short(int sm, int NT) { return (NT + 7) / 8 < RES / sm; }

// The short form's share of XCD x (= b & 7): the eight XCDs form an XN x XM grid; XCD x owns n-group x % XN and m-group x / XN.
//   natural split: XN = the smallest power of two with XN * SN >= NT (at most 8), XM = 8 / XN;
//   fewer pair rows than m-groups: XM = P and the XCDs left go to the candidate tiles, XN = min(8 / XM, NT)
//   (no group is ever empty; with XM * XN < 8 the XCDs x >= XM * XN stay idle).
// Slices are balanced: group g of n items split k ways owns [g n / k, (g + 1) n / k).
// Returns false for an idle XCD; else pairs i = p0 + j * pstep, j < R, and tiles [t0, t0 + W).
template <int RES>
GPX_MAP_FN bool sweep_short_share(int x, bool strided, int sm, int NT, int nR, int& p0, int& pstep, int& R, int& t0, int& W) {
    const int SN = RES / sm;
    const int P = (nR + 1) / 2;                // pairs (nR-1-i, i); the odd middle tile is the last one, alone
    int xn_nat = 1;
    while (xn_nat < 8 && xn_nat * SN < NT) xn_nat *= 2;
    const int xm_nat = 8 / xn_nat;
    const int XM = xm_nat < P ? xm_nat : P;
    const int XN = 8 / XM < NT ? 8 / XM : NT;
    const int xn = x % XN, xm = x / XN;
    if (xm >= XM) return false;
    t0 = (int)((long long)xn * NT / XN);
    W = (int)((long long)(xn + 1) * NT / XN) - t0;
    if (strided) {
        p0 = xm;
        pstep = XM;
        R = (P - xm + XM - 1) / XM;
    } else {
        p0 = (int)((long long)xm * P / XM);
        pstep = 1;
        R = (int)((long long)(xm + 1) * P / XM) - p0;
    }
    return true;
}

// Blocks of XCD x in the short form: its R pair rows x W tiles row by row where the slice fits a super-tile (always so where
// sweep_map_is_short holds; no idle block then), else in sm x SN patches as order 3 walks them.
template <int RES>
GPX_MAP_FN int sweep_short_depth(int sm, int R, int W) {
    const int SN = RES / sm;
    if (W <= SN) return R * W;
    return RES * ((W + SN - 1) / SN) * ((R + sm - 1) / sm);
}

// blockIdx -> tile(s) of the launch.  Returns false when the block has nothing to do; mt2 >= 0: the workgroup also
// computes tile (mt2, nt) afterwards.  RES = workgroups resident per XCD (32 CUs x workgroups per CU): the size of a super-tile.
// nP here is the number of block rows the MAP covers, [0, nP): the factor's for a full launch, the leading nR of a row-prefix
// launch (sweep_tiles) -- pairs are then (nR-1-i, i), the odd middle tile alone as ever.
template <int RES>
GPX_MAP_FN bool sweep_tile_of(int b, int order, int sm, int NT, int nP, int& mt, int& nt, int& mt2) {
    mt2 = -1;
    if (order == 1) {
        // XCD-aware: block b runs on XCD b%8 (observed, speed only).  Give each XCD its own
        // contiguous slice of candidate tiles so the tiles resident on one XCD walk the
        // SAME mt (shared T rows in that XCD's L2) over neighbouring nt.
        const int x = b & 7, q = b >> 3;          // q-th block of XCD x
        const int per = (NT + 7) / 8;             // candidate tiles per XCD
        const int lm = q / per, ln = q - lm * per;
        mt = nP - 1 - lm;
        nt = x * per + ln;
        return !(nt >= NT || mt < 0);
    }
    if (order == 2 || order == 3) {
        // XCD-aware 2-D super-tiles: the RES workgroups resident on one XCD form an sm (mt) x SN (nt) patch, so every
        // T row-panel and every Ks column-panel fetched into that XCD's L2 is used by several tiles.
        // order 3: PAIRED tiles on the super-tile map: the workgroup computes (nP-1-i, nt) and then (i, nt), so every
        // workgroup of the launch does the same (nP+1)*128 of K.  Equal durations keep the workgroups
        // of a super-tile in step for the whole launch: tiles that share a Ks column panel (same nt,
        // different mt) walk k together instead of drifting apart by their K-extent difference.
        const int x = b & 7, q = b >> 3;
        const int SN = RES / sm;                  // super-tile = sm (mt) x SN (nt) = RES workgroups
        const int per = (NT + 7) / 8;             // candidate tiles per XCD (contiguous slice)
        const int hper = (per + SN - 1) / SN;     // n-groups per XCD
        const int s = q / RES, r = q - s * RES;
        const int G = s / hper, H = s - G * hper;
        const int i = G * sm + r / SN;
        const int ln = H * SN + (r - (r / SN) * SN);
        nt = x * per + ln;
        mt = nP - 1 - i;
        if (order == 2) return !(ln >= per || nt >= NT || mt < 0);
        if (ln >= per || nt >= NT || i > mt) return false;
        if (i < mt) mt2 = i;
        return true;
    }
    if (order == SWEEP_ORDER_SHORT || order == SWEEP_ORDER_SHORT_STRIDED) {
        // short form of order 3: the same pairs, heavy rows first, on the XCD's own pair rows and its own tiles only
        const int x = b & 7, q = b >> 3;
        int p0, pstep, R, t0, W;
        if (!sweep_short_share<RES>(x, order == SWEEP_ORDER_SHORT_STRIDED, sm, NT, nP, p0, pstep, R, t0, W)) return false;
        const int SN = RES / sm;
        int li, ln;
        if (W <= SN) {
            li = q / W;
            ln = q - li * W;
        } else {
            const int hper = (W + SN - 1) / SN;
            const int s = q / RES, r = q - s * RES;
            const int G = s / hper, H = s - G * hper;
            li = G * sm + r / SN;
            ln = H * SN + (r - (r / SN) * SN);
        }
        if (li >= R || ln >= W) return false;
        const int i = p0 + li * pstep;
        nt = t0 + ln;
        mt = nP - 1 - i;                          // i < (nP + 1) / 2, so i <= mt
        if (i < mt) mt2 = i;
        return true;
    }
    mt = nP - 1 - b / NT;
    nt = b - (b / NT) * NT;
    return true;
}

// Blocks of a launch: every working block of the map lies below it.  The short forms end at their last working block.
template <int RES>
GPX_MAP_FN unsigned sweep_grid(int order, int super_m, int NT, int nP) {
    const int per = (NT + 7) / 8;
    if (order == 1) return (unsigned)(8 * per * nP);
    if (order == 2 || order == 3) {
        const int SN = RES / super_m;
        const int hper = (per + SN - 1) / SN;
        const int rows = (order == 3) ? (nP + 1) / 2 : nP;
        const int gm = (rows + super_m - 1) / super_m;
        return (unsigned)(8 * RES * hper * gm);
    }
    if (order == SWEEP_ORDER_SHORT || order == SWEEP_ORDER_SHORT_STRIDED) {
        int dmax = 0, xlast = 0;
        for (int x = 0; x < 8; ++x) {
            int p0, pstep, R, t0, W;
            if (!sweep_short_share<RES>(x, order == SWEEP_ORDER_SHORT_STRIDED, super_m, NT, nP, p0, pstep, R, t0, W)) continue;
            const int dx = sweep_short_depth<RES>(super_m, R, W);
            if (dx >= dmax) { dmax = dx; xlast = x; }
        }
        return dmax ? (unsigned)(8 * (dmax - 1) + xlast + 1) : 0u;
    }
    return (unsigned)(NT * nP);
}

}  // namespace gpx
#endif  // GPX_SWEEP_MAP_H
