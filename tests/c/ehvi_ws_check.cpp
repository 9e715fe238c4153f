// Host checker of the two-objective sweep's workspace (pybo_amd/csrc/ws_layout.h: ehvi_ws), in the scheme of con_ws_check.cpp
// (tests/test_ehvi_host.py): the walk runs over candidate counts and front sizes twice, on a null base (sizing) and on a real allocation
// of exactly that size, and prints
//     layout ehvi <shape-tag> <field> <offset> <bytes>
//     layout ehvi <shape-tag> total 0 <bytes>
// which the Python side holds against tests/golden/ehvi_ws_layouts.json.  Checked here: both walks give the same total; every region
// lies inside it; the regions are pairwise disjoint and in walk order; the four moment vectors are one (4, M) array from the base; b
// follows a directly (one upload fills both); a sizing walk hands out no pointer.
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
    const int64_t MS[5] = {1, 257, 4096, 13001, 1048576};
    const int64_t NS[4] = {0, 1, 7, 1024};
    for (int64_t M : MS)
        for (int64_t n : NS) {
            const long long m = (long long)M, nn = (long long)n;
            const EhviWs z = ehvi_ws(WsCarver(nullptr), M, n);
            const int64_t total = z.bytes;
            CHECK(!z.mom && !z.out && !z.a && !z.b, "M %lld n %lld: a sizing walk returned a pointer", m, nn);
            std::vector<WsRegion> regs;
            char* base = static_cast<char*>(aligned_alloc(4096, (size_t)((total + 4095) / 4096 * 4096 + 4096)));
            const EhviWs w = ehvi_ws(WsCarver(base, &regs), M, n);
            CHECK(w.bytes == total, "M %lld n %lld: sizing walk %lld, carving walk %lld", m, nn, (long long)total, (long long)w.bytes);
            CHECK(reinterpret_cast<char*>(w.mom) == base, "M %lld n %lld: the moments are not the base", m, nn);
            CHECK(w.out == w.mom + 4 * M && w.a == w.out + M && w.b == w.a + n + 2, "M %lld n %lld: out / a / b are not where the kernel reads them", m, nn);
            CHECK(total == (5 * M + 2 * (n + 2)) * 8, "M %lld n %lld: total %lld", m, nn, (long long)total);
            free(base);
            CHECK(regs.size() == 7, "M %lld n %lld: %zu regions", m, nn, regs.size());
            int64_t end = 0;
            for (const WsRegion& r : regs) {
                CHECK(r.offset == end && r.offset % 8 == 0 && r.bytes > 0 && r.offset + r.bytes <= total, "M %lld n %lld %s: not packed in walk order", m, nn, r.name);
                end = r.offset + r.bytes;
            }
            for (const WsRegion& r : regs) printf("layout ehvi M%lld_n%lld %s %lld %lld\n", m, nn, r.name, (long long)r.offset, (long long)r.bytes);
            printf("layout ehvi M%lld_n%lld total 0 %lld\n", m, nn, (long long)total);
            ++nlayouts;
        }
    printf("layouts %d\n", nlayouts);
    if (bad) return 1;
    printf("ws layout ok\n");
    return 0;
}
