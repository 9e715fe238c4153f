// Host checker of the constrained sweep's workspace (pybo_amd/csrc/ws_layout.h: con_ws), in the scheme of ws_layout_check.cpp
// (tests/test_con_ws_host.py): the walk runs over the candidate counts of that program twice, on a null base (sizing) and on a real
// allocation of exactly that size, and prints
//     layout con <shape-tag> <field> <offset> <bytes>
//     layout con <shape-tag> total 0 <bytes>
// which the Python side holds against tests/golden/con_ws_layouts.json.  Checked here: both walks give the same total; every region
// lies inside it; the regions are pairwise disjoint; the first pointer is the base; a sizing walk hands out no pointer.
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

int main() {
    const int64_t MS[6] = {1, 127, 1000, 4096, 13001, 32768};
    for (int64_t M : MS) {
        const long long m = (long long)M;
        const int64_t total = con_ws(WsCarver(nullptr), M).bytes;
        std::vector<WsRegion> regs;
        char* base = static_cast<char*>(aligned_alloc(4096, (size_t)((total + 4095) / 4096 * 4096 + 4096)));
        const ConWs w = con_ws(WsCarver(base, &regs), M);
        CHECK(w.bytes == total, "M %lld: sizing walk %lld, carving walk %lld", m, (long long)total, (long long)w.bytes);
        CHECK(reinterpret_cast<char*>(w.t0) == base, "M %lld: the first region is not the base", m);
        CHECK(con_ws(WsCarver(nullptr), M).t0 == nullptr && con_ws(WsCarver(nullptr), M).out == nullptr, "M %lld: a sizing walk returned a pointer", m);
        CHECK(w.out == w.t0 + M, "M %lld: the running product does not follow the probabilities", m);
        free(base);
        std::vector<WsRegion> by = regs;
        std::sort(by.begin(), by.end(), [](const WsRegion& a, const WsRegion& b) { return a.offset < b.offset; });
        int64_t end = 0;
        for (const WsRegion& r : by) {
            CHECK(r.offset >= 0 && r.bytes == M * 8 && r.offset + r.bytes <= total, "M %lld %s: out of bounds", m, r.name);
            CHECK(r.offset >= end && r.offset % 8 == 0, "M %lld %s: overlaps the region before it", m, r.name);
            end = r.offset + r.bytes;
        }
        for (const WsRegion& r : regs) printf("layout con M%lld %s %lld %lld\n", m, r.name, (long long)r.offset, (long long)r.bytes);
        printf("layout con M%lld total 0 %lld\n", m, (long long)total);
        ++nlayouts;
    }
    printf("layouts %d\n", nlayouts);
    if (bad) return 1;
    printf("ws layout ok\n");
    return 0;
}
