// sweep_map_check.cpp -- host-only proof that every block -> tile map of pybo_amd/csrc/sweep_map.h is total and exact
// (tests/test_sweep_map_host.py builds and runs it, once plainly and once with -fsanitize=address,undefined).
// For every order (0 .. 3, the short forms 4 and 5 of order 3), RES in {64, 96}, sm in {1, 2, 4, 8, 16}, NT in 1 .. 70 and 512,
// nR in 1 .. 70 the grid of sweep_grid is run through sweep_tile_of:
//   - no block yields mt < 0, mt >= nR, nt < 0, nt >= NT, or a second tile outside [0, mt);
//   - every tile (mt, nt) is produced exactly once, as a first tile or as an mt2;
//   - the paired maps pair (nR-1-i, i) and leave only the odd middle tile alone;
//   - no block behind the grid works (orders 1 .. 5; order 0 has no idle blocks and no test of its own);
//   - a short form, where launch_sweep_trmm chooses it by size, has at most as many idle blocks as working ones.
// Prints one line per order and exits 0, or prints the first violations and exits 1.
#include "../../pybo_amd/csrc/sweep_map.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

using namespace gpx;

static std::atomic<long long> g_fail{0};
static void fail(const char* what, int RES, int order, int sm, int NT, int nR, long long b, int mt, int nt, int mt2) {
    if (g_fail++ < 20)
        std::fprintf(stderr, "FAIL %s: RES %d order %d sm %d NT %d nR %d block %lld -> mt %d nt %d mt2 %d\n", what, RES, order, sm, NT,
                     nR, b, mt, nt, mt2);
}

struct Stats {
    long long cases = 0, blocks = 0, working = 0, worst_idle_num = 0, worst_idle_den = 1;
};

template <int RES>
static void check(int order, int sm, int NT, int nR, Stats& st) {
    const unsigned grid = sweep_grid<RES>(order, sm, NT, nR);
    std::vector<unsigned char> seen((size_t)NT * nR, 0);      // heap: the sanitizer build sees every index
    long long working = 0;
    const long long behind = (order == 0) ? 0 : 8LL * RES + 64;
    for (long long b = 0; b < (long long)grid + behind; ++b) {
        int mt = -12345, nt = -12345, mt2 = -12345;
        const bool works = sweep_tile_of<RES>((int)b, order, sm, NT, nR, mt, nt, mt2);
        if (!works) continue;
        if (b >= grid) { fail("a working block behind the grid", RES, order, sm, NT, nR, b, mt, nt, mt2); continue; }
        ++working;
        if (mt < 0 || mt >= nR || nt < 0 || nt >= NT) { fail("first tile out of range", RES, order, sm, NT, nR, b, mt, nt, mt2); continue; }
        if (mt2 != -1 && (mt2 < 0 || mt2 >= mt)) { fail("second tile out of range", RES, order, sm, NT, nR, b, mt, nt, mt2); continue; }
        const bool paired = order >= 3;
        if (!paired && mt2 != -1) fail("an unpaired map gave a second tile", RES, order, sm, NT, nR, b, mt, nt, mt2);
        if (paired && mt2 != -1 && mt2 != nR - 1 - mt) fail("not the pair (nR-1-i, i)", RES, order, sm, NT, nR, b, mt, nt, mt2);
        if (paired && mt2 == -1 && 2 * mt != nR - 1) fail("a lone tile that is not the middle one", RES, order, sm, NT, nR, b, mt, nt, mt2);
        if (seen[(size_t)mt * NT + nt]++) fail("tile produced twice", RES, order, sm, NT, nR, b, mt, nt, mt2);
        if (mt2 >= 0 && seen[(size_t)mt2 * NT + nt]++) fail("tile produced twice (as mt2)", RES, order, sm, NT, nR, b, mt, nt, mt2);
    }
    for (int mt = 0; mt < nR; ++mt)
        for (int nt = 0; nt < NT; ++nt)
            if (seen[(size_t)mt * NT + nt] != 1) fail("tile not produced exactly once", RES, order, sm, NT, nR, -1, mt, nt, -1);
    const long long idle = (long long)grid - working;
    if (order >= SWEEP_ORDER_SHORT && sweep_map_is_short<RES>(sm, NT)) {
        if (idle > working) fail("more idle blocks than working ones", RES, order, sm, NT, nR, grid, (int)working, (int)idle, -1);
        if (idle * st.worst_idle_den > st.worst_idle_num * working) st.worst_idle_num = idle, st.worst_idle_den = working;
    }
    ++st.cases;
    st.blocks += grid;
    st.working += working;
}

int main() {
    const int sms[] = {1, 2, 4, 8, 16};
    const int norder = SWEEP_ORDER_SHORT_STRIDED + 1, njobs = norder * 5;
    std::vector<Stats> stats(njobs);                 // job = (order, sm): the jobs share nothing but the failure count
    std::atomic<int> next{0};
    auto worker = [&]() {
        for (int job = next++; job < njobs; job = next++) {
            const int order = job / 5, sm = sms[job % 5];
            for (int nti = 1; nti <= 71; ++nti) {
                const int NT = nti <= 70 ? nti : 512;
                for (int nR = 1; nR <= 70; ++nR) {
                    check<64>(order, sm, NT, nR, stats[job]);
                    check<96>(order, sm, NT, nR, stats[job]);
                }
            }
        }
    };
    unsigned nthreads = std::thread::hardware_concurrency();
    nthreads = nthreads < 1 ? 1 : (nthreads > 8 ? 8 : nthreads);
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < nthreads; ++t) pool.emplace_back(worker);
    worker();
    for (auto& t : pool) t.join();
    for (int order = 0; order < norder; ++order) {
        Stats st;
        for (int j = order * 5; j < order * 5 + 5; ++j) {
            st.cases += stats[j].cases, st.blocks += stats[j].blocks, st.working += stats[j].working;
            if (stats[j].worst_idle_num * st.worst_idle_den > st.worst_idle_num * stats[j].worst_idle_den)
                st.worst_idle_num = stats[j].worst_idle_num, st.worst_idle_den = stats[j].worst_idle_den;
        }
        std::printf("order %d: %lld launches, %lld blocks, %lld working", order, st.cases, st.blocks, st.working);
        if (order >= SWEEP_ORDER_SHORT) std::printf(", worst idle / working of a short launch chosen by size %lld / %lld", st.worst_idle_num, st.worst_idle_den);
        std::printf("\n");
    }
    // the shapes the short form was designed on: NT = 16, nR = 64, sm = 8 -> 8 pair rows x 8 tiles on every XCD and no idle block
    if (sweep_grid<64>(SWEEP_ORDER_SHORT, 8, 16, 64) != 512u) { std::fprintf(stderr, "FAIL grid of NT 16 nR 64\n"); ++g_fail; }
    if (sweep_grid<64>(SWEEP_ORDER_SHORT, 8, 1, 64) != 8u * 3 + 8) { std::fprintf(stderr, "FAIL grid of NT 1 nR 64\n"); ++g_fail; }
    if (g_fail) { std::fprintf(stderr, "%lld violations\n", (long long)g_fail); return 1; }
    std::printf("sweep maps ok\n");
    return 0;
}
