// Host checker of the pathwise Thompson draws' workspaces (pybo_amd/csrc/ws_layout.h: path_sweep_ws, path_weights_ws, path_grad_ws and
// the fragment-order panel's arithmetic), in the scheme of ehvi_ws_check.cpp (tests/test_path_host.py): every walk runs twice, on a null
// base (sizing) and on a real allocation of exactly that size, and prints
//     layout <walk> <shape-tag> <field> <offset> <bytes>
//     layout <walk> <shape-tag> total 0 <bytes>
// which the Python side holds against tests/golden/path_ws_layouts.json.  Checked here: both walks give the same total; every region lies
// inside it, on an 8-byte boundary, disjoint from the others and in walk order; a sizing walk hands out no pointer; the panel and the
// panels of 128 draws start on 512-byte boundaries; the groups of the panel tile it exactly (every fragment index a launch of
// k_path_update reads lies inside its group, the last group ends at path_frag_words) and every padded row a workgroup walks exists in a
// factor of Np = 128 ceil(N / 128) rows.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../pybo_amd/csrc/ws_layout.h"

using namespace gpx;

static int bad = 0, nlayouts = 0;
#define CHECK(cond, ...)                                \
    do {                                                \
        if (!(cond)) {                                  \
            printf("FAILED %s: ", #cond);               \
            printf(__VA_ARGS__);                        \
            printf("\n");                               \
            ++bad;                                      \
        }                                               \
    } while (0)

static void regions(const char* walk, const char* tag, const std::vector<WsRegion>& regs, int64_t total) {
    int64_t end = 0;
    for (const WsRegion& r : regs) {
        CHECK(r.offset >= end && r.offset % 8 == 0 && r.bytes >= 0 && r.offset + r.bytes <= total, "%s %s %s: not in walk order inside the total", walk, tag, r.name);
        end = r.offset + r.bytes;
        printf("layout %s %s %s %lld %lld\n", walk, tag, r.name, (long long)r.offset, (long long)r.bytes);
    }
    printf("layout %s %s total 0 %lld\n", walk, tag, (long long)total);
    ++nlayouts;
}

static char* alloc_for(int64_t total) { return static_cast<char*>(aligned_alloc(4096, (size_t)((total + 4095) / 4096 * 4096 + 4096))); }

int main() {
    char tag[96];
    // the sweep's panel: draws around the group and block edges, rows around the tile edges
    const int64_t SS[7] = {1, 5, 16, 17, 64, 65, 130};
    const int64_t NV[6] = {1, 63, 64, 65, 127, 300};
    for (int64_t S : SS)
        for (int64_t nv : NV) {
            snprintf(tag, sizeof tag, "S%lld_nv%lld", (long long)S, (long long)nv);
            const PathSweepWs z = path_sweep_ws(WsCarver(nullptr), S, nv);
            CHECK(!z.v && !z.frag, "%s: a sizing walk returned a pointer", tag);
            std::vector<WsRegion> regs;
            char* base = alloc_for(z.bytes);
            const PathSweepWs w = path_sweep_ws(WsCarver(base, &regs), S, nv);
            CHECK(w.bytes == z.bytes, "%s: sizing walk %lld, carving walk %lld", tag, (long long)z.bytes, (long long)w.bytes);
            CHECK(reinterpret_cast<char*>(w.v) == base && (reinterpret_cast<char*>(w.frag) - base) % 512 == 0, "%s: v / frag misplaced", tag);
            CHECK(reinterpret_cast<char*>(w.frag) - base >= S * nv * 8, "%s: the panel overlaps the weights", tag);
            // the groups tile the panel: group g starts where g full groups end, and what its launch reads stays inside it
            const int64_t G = (S + PATH_GROUP - 1) / PATH_GROUP, ntile = path_tiles(nv), words = path_frag_words(S, nv);
            CHECK(ntile * PATH_ROWS >= nv && (ntile - 1) * PATH_ROWS < nv, "%s: tiles", tag);
            CHECK(ntile * PATH_ROWS <= (nv + 127) / 128 * 128, "%s: a workgroup would walk rows the factor's inputs do not have", tag);
            int64_t end = 0, draws = 0;
            for (int64_t g = 0; g < G; ++g) {
                const int njb = path_group_blocks(S, g);
                CHECK(njb >= 1 && njb <= PATH_GROUP / 16, "%s: group %lld has %d blocks", tag, (long long)g, njb);
                CHECK(path_group_offset(nv, g) == end, "%s: group %lld starts at %lld, the one before ends at %lld", tag, (long long)g,
                      (long long)path_group_offset(nv, g), (long long)end);
                // the last fragment word lane 63 reads: tile ntile - 1, k-step 15, block njb - 1
                const int64_t last = ((ntile - 1) * (PATH_ROWS / 4) * njb + ((PATH_ROWS / 4 - 1) * njb + njb - 1)) * 64 + 63;
                end += ntile * (PATH_ROWS / 4) * njb * 64;
                CHECK(path_group_offset(nv, g) + last == end - 1, "%s: group %lld is read up to %lld, ends at %lld", tag, (long long)g, (long long)last, (long long)end);
                draws += 16 * njb;
            }
            CHECK(end == words && draws >= S && draws < S + 16, "%s: the groups hold %lld words for %lld draws, the panel %lld", tag, (long long)end,
                  (long long)draws, (long long)words);
            free(base);
            regions("path_sweep", tag, regs, z.bytes);
        }
    // the weights' panels of 128 draws
    const int64_t WS[4] = {1, 5, 128, 129};
    const int64_t NN[4] = {1, 129, 300, 16384};
    for (int64_t S : WS)
        for (int64_t N : NN)
            for (int eps = 0; eps < 2; ++eps) {
                const int64_t Np = (N + NB - 1) / NB * NB, Sp = (S + TBH - 1) / TBH * TBH;
                snprintf(tag, sizeof tag, "S%lld_N%lld_eps%d", (long long)S, (long long)N, eps);
                const PathWeightsWs z = path_weights_ws(WsCarver(nullptr), S, N, Np, Sp, eps != 0);
                CHECK(!z.prior && !z.eps && !z.R && !z.V && !z.W && !z.v, "%s: a sizing walk returned a pointer", tag);
                std::vector<WsRegion> regs;
                char* base = alloc_for(z.bytes);
                const PathWeightsWs w = path_weights_ws(WsCarver(base, &regs), S, N, Np, Sp, eps != 0);
                CHECK(w.bytes == z.bytes, "%s: sizing walk %lld, carving walk %lld", tag, (long long)z.bytes, (long long)w.bytes);
                CHECK((w.eps != nullptr) == (eps != 0) && (!eps || w.eps == w.prior + S * N), "%s: eps", tag);
                CHECK((reinterpret_cast<char*>(w.R) - base) % 512 == 0 && w.V == w.R + Np * Sp && w.W == w.V + Np * Sp && w.v == w.W + Np * Sp, "%s: panels", tag);
                CHECK(reinterpret_cast<char*>(w.v + S * N) - base == w.bytes, "%s: v does not end the allocation", tag);
                free(base);
                regions("path_weights", tag, regs, z.bytes);
            }
    // one draw's value and gradient
    const int64_t GM[3] = {1, 17, 4096};
    const int64_t GD[2] = {2, 20};
    for (int64_t M : GM)
        for (int64_t d : GD) {
            const int64_t n = 100 + d, nv = 127, Np = 128;
            snprintf(tag, sizeof tag, "M%lld_d%lld", (long long)M, (long long)d);
            const PathGradWs z = path_grad_ws(WsCarver(nullptr), n, d, nv, Np, M);
            CHECK(!z.W && !z.v && !z.ks && !z.out, "%s: a sizing walk returned a pointer", tag);
            std::vector<WsRegion> regs;
            char* base = alloc_for(z.bytes);
            const PathGradWs w = path_grad_ws(WsCarver(base, &regs), n, d, nv, Np, M);
            CHECK(w.bytes == z.bytes && regs.size() == 9, "%s: walks disagree", tag);
            CHECK(w.g == w.ks + GB * Np && w.part == w.g + GB * Np && w.out == w.part + GB * (2 + 2 * d), "%s: the passes' buffers", tag);
            CHECK(z.bytes == 8 * (n * d + 2 * n + nv + M * d + 2 * GB * Np + GB * (2 + 2 * d) + M * (d + 1)), "%s: total", tag);
            free(base);
            regions("path_grad", tag, regs, z.bytes);
        }
    printf("layouts %d\n", nlayouts);
    if (bad) return 1;
    printf("ws layout ok\n");
    return 0;
}
