// sweep_shape_check.cpp -- host-only check of the launch-shape rule of pybo_amd/csrc/sweep_map.h: sweep_shape_of (tile width and LDS
// images of a launch of the default sweep schedule), tests/test_sweep_shape_host.py builds and runs it, once plainly and once with
// -fsanitize=address,undefined.  argv[1]: tests/golden/sweep_cols_full_launch.txt, the widths of full launches before the image count
// existed.  Walked: nP in 1 .. 130, nR in {nP, nP / 4, 1}, valid in 1 .. 20000 around every multiple of 32 (every tile boundary of every
// width) and at the headline's list lengths, 256 and 304 compute units, the options sweep_cols in {-1, 128, 64, 32} x sweep_images in
// {-1, 1, 2}; tile order 19 at every valid, the other orders of the table at the thresholds of the rule.
//   - width in {32, 64, 128}, images in {1, 2};
//   - images = 2 by size only where the working blocks of the launch's map -- counted by walking sweep_tile_of -- are at most the CUs
//     and no XCD holds more than an eighth of the CUs, and, on map 3 of the default k-loop over at least SWEEP_NARROW_MIN_NP block
//     rows, everywhere that is so;
//   - sweep_images = 1: the width of a full launch is the table's;
//   - forced options are honoured on the default k-loop and ignored on every other;
//   - a row-prefix launch by size takes the width its costs say (sweep_prefix_cost: a narrower tile only where it costs at least 5 % less
//     and never where a wider one costs no more), the wide single-image tile below SWEEP_NARROW_MIN_NP block rows;
//   - the grid every shape implies (RES 64 for one image, 32 for two; the map sweep_order_of picks) is total and exact: every tile
//     once, none out of range, no working block behind the grid -- the walk of sweep_map_check.cpp, here at the sizes the rule produces.
// Prints a summary and exits 0, or prints the first violations and exits 1.
#include "../../pybo_amd/csrc/sweep_map.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <tuple>
#include <vector>

using namespace gpx;

static long long g_fail = 0;
#define FAIL(...) do { if (g_fail++ < 20) { std::fprintf(stderr, "FAIL " __VA_ARGS__); std::fprintf(stderr, "\n"); } } while (0)

struct Row { int to, sc, nPlo, nPhi, vlo, vhi, width; };
static std::vector<Row> g_table;

static int table_width(int to, int sc, int nP, long long valid) {
    for (const Row& r : g_table)
        if (r.to == to && r.sc == sc && nP >= r.nPlo && nP <= r.nPhi && valid >= r.vlo && valid <= r.vhi) return r.width;
    return -1;
}

// the walk of sweep_map_check.cpp: working blocks of the grid, every tile exactly once; returns the working blocks
template <int RES>
static long long walk(int order, int sm, int NT, int nR) {
    const unsigned grid = sweep_grid<RES>(order, sm, NT, nR);
    std::vector<unsigned char> seen((size_t)NT * nR, 0);
    long long working = 0;
    const long long behind = (order == 0) ? 0 : 8LL * RES + 64;
    for (long long b = 0; b < (long long)grid + behind; ++b) {
        int mt = -12345, nt = -12345, mt2 = -12345;
        if (!sweep_tile_of<RES>((int)b, order, sm, NT, nR, mt, nt, mt2)) continue;
        if (b >= grid) { FAIL("a working block behind the grid: RES %d order %d sm %d NT %d nR %d block %lld", RES, order, sm, NT, nR, b); continue; }
        ++working;
        if (mt < 0 || mt >= nR || nt < 0 || nt >= NT) { FAIL("first tile out of range: RES %d order %d NT %d nR %d block %lld", RES, order, NT, nR, b); continue; }
        if (mt2 != -1 && (mt2 < 0 || mt2 >= mt)) { FAIL("second tile out of range: RES %d order %d NT %d nR %d block %lld", RES, order, NT, nR, b); continue; }
        if (seen[(size_t)mt * NT + nt]++) FAIL("tile produced twice: RES %d order %d NT %d nR %d (%d, %d)", RES, order, NT, nR, mt, nt);
        if (mt2 >= 0 && seen[(size_t)mt2 * NT + nt]++) FAIL("tile produced twice (as mt2): RES %d order %d NT %d nR %d (%d, %d)", RES, order, NT, nR, mt2, nt);
    }
    for (size_t i = 0; i < seen.size(); ++i)
        if (seen[i] != 1) { FAIL("tile not produced exactly once: RES %d order %d sm %d NT %d nR %d tile %zu", RES, order, sm, NT, nR, i); break; }
    return working;
}

static std::set<std::tuple<int, int, int, int, int>> g_walked;      // RES, order, sm, NT, nR -> walked already
static long long g_walks = 0;
static long long walked(int images, int order0, int short_map, int sm, int NT, int nR) {
    const int RES = images == 2 ? 32 : 64;
    const int order = images == 2 ? sweep_order_of<32>(order0, short_map, sm, NT) : sweep_order_of<64>(order0, short_map, sm, NT);
    const long long working = sweep_working(order0, NT, nR);
    if (!g_walked.insert(std::make_tuple(RES, order, sm, NT, nR)).second) return working;
    ++g_walks;
    const long long w = RES == 32 ? walk<32>(order, sm, NT, nR) : walk<64>(order, sm, NT, nR);
    if (w != working) FAIL("sweep_working %lld, the map's walk %lld: RES %d order %d sm %d NT %d nR %d", working, w, RES, order, sm, NT, nR);
    return w;
}

// the most working blocks any XCD (block b runs on XCD b % 8) holds in the two-image launch's map, by walking it
static long long xcd_walk(int order0, int short_map, int sm, int NT, int nR) {
    const int order = sweep_order_of<32>(order0, short_map, sm, NT);
    static std::map<std::tuple<int, int, int, int>, long long> known;
    const auto key = std::make_tuple(order, sm, NT, nR);
    const auto it = known.find(key);
    if (it != known.end()) return it->second;
    long long per[8] = {0, 0, 0, 0, 0, 0, 0, 0}, worst = 0;
    const unsigned grid = sweep_grid<32>(order, sm, NT, nR);
    for (unsigned b = 0; b < grid; ++b) {
        int mt, nt, mt2;
        if (sweep_tile_of<32>((int)b, order, sm, NT, nR, mt, nt, mt2)) ++per[b & 7];
    }
    for (int x = 0; x < 8; ++x) worst = per[x] > worst ? per[x] : worst;
    known[key] = worst;
    return worst;
}

static bool is_width(int w) { return w == 32 || w == 64 || w == 128; }

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: sweep_shape_check tests/golden/sweep_cols_full_launch.txt\n"); return 2; }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char line[256];
    while (std::fgets(line, sizeof line, f)) {
        Row r;
        if (line[0] == '#') continue;
        if (std::sscanf(line, "%d %d %d %d %d %d %d", &r.to, &r.sc, &r.nPlo, &r.nPhi, &r.vlo, &r.vhi, &r.width) == 7) g_table.push_back(r);
    }
    std::fclose(f);
    if (g_table.size() < 40) { std::fprintf(stderr, "the table has %zu rows\n", g_table.size()); return 2; }

    std::vector<long long> valids;
    valids.push_back(1);
    valids.push_back(2);
    for (long long v = 32; v <= 20000; v += 32) { valids.push_back(v - 1); valids.push_back(v); if (v < 20000) valids.push_back(v + 1); }      // every boundary of every width
    const long long named[] = {2048, 4096, 4824, 7501, 9293, 12288, 16384, 20000};
    for (long long v : named) valids.push_back(v);
    const int tos[] = {-1, 3, 7, 15, 16, 17, 18, 19, 23, 27, 31, 51};
    const int scs[] = {-1, 128, 64, 32}, sis[] = {-1, 1, 2}, cuss[] = {256, 304};
    const int sm = 8, short_map = -1;                   // the defaults of the library
    long long cases = 0, two = 0, prefix_narrow = 0;
    for (int nP = 1; nP <= 130; ++nP) {
        const int nRs[3] = {nP, nP / 4 > 0 ? nP / 4 : 1, 1};
        for (int ri = 0; ri < 3; ++ri) {
            const int nR = nRs[ri];
            if (ri > 0 && (nR == nRs[ri - 1] || nR == nRs[0])) continue;
            for (long long valid : valids) {
                // the walks cost a grid each: every shape at the thresholds and the named lists, the two-image shapes chosen by size everywhere
                const bool walk_all = valid <= 2 || (valid >= 31 && valid <= 33) || (valid >= 255 && valid <= 257) || (valid >= 511 && valid <= 513) ||
                                      (valid >= 1023 && valid <= 1025) || valid == 2048 || valid == 4824 || valid == 9293 || valid == 20000;
                for (int to : tos) {
                    if (to != 19 && !walk_all) continue;
                    for (int cus : cuss)
                        for (int sc : scs)
                            for (int si : sis) {
                                const SweepShape s = sweep_shape_of(to, nP, nR, valid, cus, sc, si, sm, short_map);
                                ++cases;
                                if (!is_width(s.width) || (s.images != 1 && s.images != 2)) { FAIL("shape %d x %d: to %d nP %d nR %d valid %lld", s.width, s.images, to, nP, nR, valid); continue; }
                                const bool dflt = to >= 0 && ((to >> 2) & 7) == 4 && (to >> 5) == 0;      // the default k-loop: where the instances are
                                const bool by_size = dflt && (to & 3) == 3 && nP >= SWEEP_NARROW_MIN_NP;
                                const int NT = (int)((valid + s.width - 1) / s.width);
                                if (!dflt && (s.width != 128 || s.images != 1)) FAIL("a shape without instances: to %d sc %d si %d -> %d x %d", to, sc, si, s.width, s.images);
                                if (dflt && sc > 0 && s.width != sc) FAIL("forced width %d ignored: to %d nP %d nR %d valid %lld -> %d", sc, to, nP, nR, valid, s.width);
                                if (dflt && si > 0 && s.images != si) FAIL("forced images %d ignored: to %d nP %d nR %d valid %lld -> %d", si, to, nP, nR, valid, s.images);
                                if (dflt && sc < 0 && !by_size && s.width != 128) FAIL("narrow by size outside the rule: to %d nP %d nR %d valid %lld", to, nP, nR, valid);
                                if (si == 1 && nR == nP) {
                                    const int want = table_width(to, sc, nP, valid);
                                    if (want != s.width) FAIL("width %d, the table says %d: to %d sc %d nP %d valid %lld", s.width, want, to, sc, nP, valid);
                                }
                                if (si < 0) {
                                    if (s.images == 2) {
                                        ++two;
                                        if (!by_size) FAIL("two images by size outside the rule: to %d nP %d nR %d valid %lld", to, nP, nR, valid);
                                        const long long w = walked(2, to & 3, short_map, sm, NT, nR);
                                        if (w > cus) FAIL("two images for %lld working blocks on %d CUs: to %d nP %d nR %d valid %lld width %d", w, cus, to, nP, nR, valid, s.width);
                                    } else if (by_size && sweep_working(to & 3, NT, nR) <= cus && 8 * sweep_xcd_load<32>(short_map, sm, NT, nR) <= cus) {
                                        FAIL("one image where no workgroup has a partner or waits: to %d nP %d nR %d valid %lld width %d cus %d", to, nP, nR, valid, s.width, cus);
                                    }
                                    if (s.images == 2 && 8 * xcd_walk(to & 3, short_map, sm, NT, nR) > cus)
                                        FAIL("two images although an XCD holds more than its share: to %d nP %d nR %d valid %lld width %d cus %d", to, nP, nR, valid, s.width, cus);
                                }
                                if (by_size && sc < 0 && nR != nP) {
                                    // the prefix rule: the wide tile unless a narrower one costs at least 5 % less than the best wider one
                                    int want = 128;
                                    for (int W = 64; W >= SWEEP_PREFIX_MIN_W; W /= 2)
                                        if (sweep_prefix_cost(short_map, sm, nR, valid, W) * 100 < sweep_prefix_cost(short_map, sm, nR, valid, want) * 95) want = W;
                                    if (s.width != want) FAIL("prefix width %d, by its costs %d: nP %d nR %d valid %lld", s.width, want, nP, nR, valid);
                                    for (int W = 128; W > s.width; W /= 2)
                                        if (sweep_prefix_cost(short_map, sm, nR, valid, W) <= sweep_prefix_cost(short_map, sm, nR, valid, s.width))
                                            FAIL("prefix width %d although %d costs no more: nP %d nR %d valid %lld", s.width, W, nP, nR, valid);
                                    if (s.width < 128) ++prefix_narrow;
                                }
                                if (dflt && cus == 256 && walk_all && (long long)NT * nR <= 400000) walked(s.images, to & 3, short_map, sm, NT, nR);
                            }
                }
            }
        }
    }
    // the per-XCD load the prefix rule counts is the map's: compared with a walk at the headline's shapes
    for (int W = 128; W >= 32; W /= 2) {
        const int NT = (9293 + W - 1) / W, nR = 16;
        const int order = sweep_order_of<64>(3, short_map, sm, NT);
        long long per[8] = {0, 0, 0, 0, 0, 0, 0, 0}, worst = 0;
        for (unsigned b = 0; b < sweep_grid<64>(order, sm, NT, nR); ++b) {
            int mt, nt, mt2;
            if (sweep_tile_of<64>((int)b, order, sm, NT, nR, mt, nt, mt2)) ++per[b & 7];
        }
        for (int x = 0; x < 8; ++x) worst = per[x] > worst ? per[x] : worst;
        if (worst != sweep_xcd_load<64>(short_map, sm, NT, nR)) FAIL("sweep_xcd_load %lld, the walk %lld at width %d", sweep_xcd_load<64>(short_map, sm, NT, nR), worst, W);
    }
    if (sweep_xcd_load<64>(-1, 8, 73, 16) != 80 || sweep_xcd_load<64>(-1, 8, 146, 16) != 152) FAIL("the headline's prefix launch: 80 and 152 workgroups per XCD expected");
    // the headline workloads' prefix launches (nR = 16): the widths the measured table says
    {
        const long long lists[] = {2048, 4096, 4824, 7501, 9293, 12288, 16384};
        const int best[] = {32, 64, 32, 128, 64, 128, 128};
        for (int i = 0; i < 7; ++i) {
            const SweepShape s = sweep_shape_of(19, 64, 16, lists[i], 256, -1, -1, 8, -1);
            if (s.width != best[i] || s.images != 1) FAIL("prefix launch of %lld columns: %d x %d, measured best %d x 1", lists[i], s.width, s.images, best[i]);
        }
    }
    // the headline's two short launches (N = 8192: 64 block rows, 256 seeds and 158 second-level survivors) take two images 32 wide
    for (long long v : {256LL, 158LL, 93LL}) {
        const SweepShape s = sweep_shape_of(19, 64, 64, v, 256, -1, -1, 8, -1);
        if (s.width != 32 || s.images != 2) FAIL("headline launch of %lld columns: %d x %d", v, s.width, s.images);
    }
    if (g_fail) { std::fprintf(stderr, "%lld violations\n", g_fail); return 1; }
    std::printf("%lld shapes, %lld with two images by size, %lld narrow row-prefix launches by size, %lld grids walked\n", cases, two, prefix_narrow, g_walks);
    std::printf("sweep shapes ok\n");
    return 0;
}
