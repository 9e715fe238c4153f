// Host checker of the fantasised batch proposals' workspace (pybo_amd/csrc/ws_layout.h: fant_ws), in the scheme of ws_layout_check.cpp
// (tests/test_fant_ws_host.py): the walk runs at (M, nb, S) = (1, 1, 1), (3001, 8, 5), (2^20, 64, 64) -- M does not enter it: everything
// per candidate lives in the believer's batch_ws, whose recorded layout tests/test_ws_layout_host.py pins -- twice, on a null base
// (sizing) and on a real allocation of exactly that size, and prints
//     layout fant <shape-tag> <field> <offset> <bytes>
//     layout fant <shape-tag> total 0 <bytes>
// which the Python side holds against tests/golden/fant_ws_layouts.json.  Checked here: both walks give the same total; every region lies
// inside it; the regions are pairwise disjoint and aligned to their element type; what the readers need: the innovations start at the
// base and every pick's row of Sp doubles, hence every chunk of FANT_CHUNK fantasies, on a 128-byte boundary; the incumbents follow the
// rows directly (one copy into LDS takes the rows, a second the incumbents); 64 forced rows; S <= Sp < S + FANT_CHUNK.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

int main() {
    const int64_t SHAPES[3][3] = {{1, 1, 1}, {3001, 8, 5}, {(int64_t)1 << 20, 64, 64}};
    for (const auto& sh : SHAPES) {
        const int64_t M = sh[0], nb = sh[1], S = sh[2];      // (M: the tag only)
        char tag[64];
        snprintf(tag, sizeof tag, "M%lld_nb%lld_S%lld", (long long)M, (long long)nb, (long long)S);
        const FantWs size = fant_ws(WsCarver(nullptr), nb, S);
        const int64_t total = size.bytes, rows = nb > 1 ? nb - 1 : 1;
        CHECK(size.eps == nullptr && size.t == nullptr && size.pend == nullptr, "%s: a sizing walk returned a pointer", tag);
        std::vector<WsRegion> regs;
        CHECK(total % 128 == 0, "%s: the total is not a multiple of 128 bytes", tag);
        char* base = static_cast<char*>(aligned_alloc(128, (size_t)total));      // exactly the size: the sanitizer build sees a write past it
        const FantWs w = fant_ws(WsCarver(base, &regs), nb, S);
        CHECK(w.bytes == total, "%s: sizing walk %lld, carving walk %lld", tag, (long long)total, (long long)w.bytes);
        CHECK(w.Sp == size.Sp && w.Sp >= S && w.Sp < S + FANT_CHUNK && w.Sp % FANT_CHUNK == 0 && w.Sp <= FANT_MAX_S, "%s: Sp = %lld", tag, (long long)w.Sp);
        CHECK(reinterpret_cast<char*>(w.eps) == base, "%s: the first region is not the base", tag);
        CHECK((w.Sp * 8) % 128 == 0, "%s: a pick's row of innovations is not a multiple of 128 bytes", tag);
        CHECK(w.t == w.eps + rows * w.Sp, "%s: the incumbents do not follow the innovations", tag);
        CHECK((reinterpret_cast<char*>(w.t) - base) % 128 == 0, "%s: the incumbents are off the 128-byte boundary", tag);
        CHECK(reinterpret_cast<char*>(w.pend) == reinterpret_cast<char*>(w.t + w.Sp), "%s: the forced rows do not follow the incumbents", tag);
        // the kernels' furthest reads: row nb - 2 of the innovations up to column Sp - 1, incumbent Sp - 1, forced row nb - 2 < 64
        memset(base, 0, (size_t)total);
        w.eps[(rows - 1) * w.Sp + w.Sp - 1] = 1.0, w.t[w.Sp - 1] = 1.0, w.pend[63] = 1;
        free(base);
        std::vector<WsRegion> by = regs;
        std::sort(by.begin(), by.end(), [](const WsRegion& a, const WsRegion& c) { return a.offset < c.offset; });
        int64_t end = 0;
        for (const WsRegion& r : by) {
            CHECK(r.offset >= 0 && r.bytes > 0 && r.offset + r.bytes <= total, "%s %s: out of bounds", tag, r.name);
            CHECK(r.offset >= end && r.offset % 8 == 0, "%s %s: overlaps the region before it", tag, r.name);
            end = r.offset + r.bytes;
        }
        CHECK(regs.size() == 3 && end == total, "%s: %d regions, the last ends at %lld of %lld", tag, (int)regs.size(), (long long)end, (long long)total);
        for (const WsRegion& r : regs) printf("layout fant %s %s %lld %lld\n", tag, r.name, (long long)r.offset, (long long)r.bytes);
        printf("layout fant %s total 0 %lld\n", tag, (long long)total);
        ++nlayouts;
    }
    printf("layouts %d\n", nlayouts);
    if (bad) return 1;
    printf("ws layout ok\n");
    return 0;
}
