// sweep_map.h -- block -> tile maps of the dominant sweep kernel (kernels_sweep.hip: sweep_tiles), the grid of a launch, and the shape
// of a launch's tiles (sweep_shape_of: width and LDS images).  Plain C++ without HIP types: the device code and the host launch share
// it, and tests/c/sweep_map_check.cpp and tests/c/sweep_shape_check.cpp compile it into host-only programs that walk every grid and
// every shape and prove each map total and exact, and the rule what it says, before a launch relies on them.
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

// the map of a launch: order 3 in its short form where the option short_map and the launch's size say so
// (short_map: -1 where the launch cannot fill the per-XCD patches, 0 never, 1 always, 2 the strided short form)
template <int RES>
GPX_MAP_FN int sweep_order_of(int order, int short_map, int sm, int NT) {
    if (order != 3 || short_map == 0) return order;
    if (short_map < 0 && !sweep_map_is_short<RES>(sm, NT)) return order;
    return short_map == 2 ? SWEEP_ORDER_SHORT_STRIDED : SWEEP_ORDER_SHORT;
}

// ---- the shape of a launch of the default schedule: tile width and LDS images ------------------------------------------------
// Width W = 128, 64 or 32 candidates per tile (narrow tiles: kernels_sweep.hip, sweep_tiles), images = 1 (gemm_tile_128_l, two
// workgroups per CU) or 2 (gemm_tile_128_l2, one per CU).  Every shape writes the same bits; the choice is about time alone.
// By size, launches leave the wide single-image tile from this many block rows of the factor on only (api.hip, PRUNE_SEEDS_MIN_NP: why)
constexpr int SWEEP_NARROW_MIN_NP = 48;
constexpr long long SWEEP_COLS32_MAX = 512, SWEEP_COLS64_MAX = 1024;     // full launches: profiles/narrow_seeds_ab.md, section 1
constexpr int SWEEP_PREFIX_MIN_W = 32;                                  // the narrowest tile a row-prefix launch takes by size
struct SweepShape { int width, images; };

// working workgroups of a launch of NT tiles over nR block rows: one per tile, in the paired maps one per pair or lone middle tile
GPX_MAP_FN long long sweep_working(int order, int NT, int nR) { return (long long)NT * (order == 3 ? (nR + 1) / 2 : nR); }

// The most working workgroups any XCD holds in a launch of map 3 (in the form sweep_order_of<RES> picks) of NT tiles over nR block rows
template <int RES>
GPX_MAP_FN long long sweep_xcd_load(int short_map, int sm, int NT, int nR) {
    const int P = (nR + 1) / 2;
    const int order = sweep_order_of<RES>(3, short_map, sm, NT);
    long long worst = 0;
    for (int x = 0; x < 8; ++x) {
        long long wx;
        if (order == 3) {
            const int per = (NT + 7) / 8;                  // the XCD's slice of candidate tiles, all pair rows
            const int t0 = x * per;
            wx = (long long)P * (t0 >= NT ? 0 : (NT - t0 < per ? NT - t0 : per));
        } else {
            int p0, pstep, R, t0, W;
            wx = sweep_short_share<RES>(x, order == SWEEP_ORDER_SHORT_STRIDED, sm, NT, nR, p0, pstep, R, t0, W) ? (long long)R * W : 0;
        }
        if (wx > worst) worst = wx;
    }
    return worst;
}

// Row-prefix launches (nR < nP, single image, 64 workgroups resident per XCD): the width whose workgroups fill whole generations
// best.  A launch takes as long as its fullest XCD.  Its cost in units of 1 / 2000 of a wide generation: per full generation of 64
// workgroups 20, for a last one of up to 32 (one per CU: nobody shares the matrix pipe) 12, times W / 32, times what a narrow
// tile's shorter k-steps lose at two workgroups per CU (100 / 105 / 115 at W = 128 / 64 / 32).  The figures are the prefix table
// of profiles/exact_launch_images_ab.md (nR = 16, 2048 .. 16384 columns).
GPX_MAP_FN long long sweep_prefix_cost(int short_map, int sm, int nR, long long valid, int W) {
    const long long load = sweep_xcd_load<64>(short_map, sm, (int)((valid + W - 1) / W), nR);
    const long long rem = load % 64;
    const long long units = load / 64 * 20 + (rem == 0 ? 0 : rem <= 32 ? 12 : 20);
    return units * (W / 32) * (W == 128 ? 100 : W == 64 ? 105 : 115);
}
// The wide tile unless a narrower one costs at least 5 % less than the best wider one (ties and near-ties: the wide tile).
GPX_MAP_FN int sweep_prefix_width(int short_map, int sm, int nR, long long valid) {
    int best = 128;
    long long best_cost = sweep_prefix_cost(short_map, sm, nR, valid, 128);
    for (int W = 64; W >= SWEEP_PREFIX_MIN_W; W /= 2) {
        const long long cost = sweep_prefix_cost(short_map, sm, nR, valid, W);
        if (cost * 100 < best_cost * 95) best = W, best_cost = cost;
    }
    return best;
}

// tile_order: the launch's (bits 0-1 map, bits 2-4 k-loop, above: probe builds' cache policy); nP: the factor's block rows; nR <= nP: the
// block rows the launch covers; valid: its candidate columns; cus: the device's compute units; sweep_cols, sweep_images: the options
// (-1: by size; else forced wherever instances exist, i.e. on the default k-loop); sm, short_map: the launch's super_m and short_map.
// By size (map 3 over at least SWEEP_NARROW_MIN_NP block rows; wide, one image everywhere else):
//   width   full launches: 32 up to 512 columns, 64 up to 1024, 128 beyond; row-prefix launches: sweep_prefix_width
//   images  2 exactly where the launch's working workgroups number at most the compute units, and no XCD's share of them (block b
//           runs on XCD b % 8) more than its eighth of the units: no workgroup would have a partner on its CU, none waits for a slot
GPX_MAP_FN SweepShape sweep_shape_of(int tile_order, int nP, int nR, long long valid, int cus, int sweep_cols, int sweep_images, int sm,
                                     int short_map) {
    SweepShape s = {128, 1};
    if (tile_order < 0 || ((tile_order >> 2) & 7) != 4 || (tile_order >> 5) != 0) return s;       // instances: the default k-loop only
    const int order0 = tile_order & 3;
    const bool by_size = nP >= SWEEP_NARROW_MIN_NP && order0 == 3;
    if (sweep_cols > 0) s.width = sweep_cols;
    else if (by_size) s.width = nR != nP ? sweep_prefix_width(short_map, sm, nR, valid) : valid <= SWEEP_COLS32_MAX ? 32 : valid <= SWEEP_COLS64_MAX ? 64 : 128;
    if (sweep_images > 0) s.images = sweep_images;
    else if (by_size) {
        const int NT = (int)((valid + s.width - 1) / s.width);
        if (sweep_working(order0, NT, nR) <= cus && 8 * sweep_xcd_load<32>(short_map, sm, NT, nR) <= cus) s.images = 2;
    }
    return s;
}

}  // namespace gpx
#endif  // GPX_SWEEP_MAP_H
