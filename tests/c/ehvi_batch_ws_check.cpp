// Host checker of what the two-objective batch adds to the lead's scratch (pybo_amd/csrc/ws_layout.h: ehvi_batch_ws), in the scheme of
// ehvi_ws_check.cpp (tests/test_ehvi_insert_host.py): the walk runs twice per pitch, on a null base (sizing) and on a real allocation of
// exactly that size, and prints
//     layout ehvi_batch <shape-tag> <field> <offset> <bytes>
//     layout ehvi_batch <shape-tag> total 0 <bytes>
// which the Python side holds against tests/golden/ehvi_batch_ws_layouts.json.  Checked here: both walks give the same total; the regions
// are packed in walk order, 8-byte aligned, inside the total; b follows a directly (one upload fills both); the pitch the library uses,
// EHVI_STRIP_LD, holds a front at the cap with the word an insertion may add; a sizing walk hands out no pointer.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../pybo_amd/csrc/ehvi_math.h"
#include "../../pybo_amd/csrc/ws_layout.h"

using namespace gpx;

static int bad = 0, nlayouts = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            printf("FAILED %s: ", #cond); \
            printf(__VA_ARGS__);          \
            printf("\n");                 \
            ++bad;                        \
        }                                 \
    } while (0)

int main() {
    static_assert(EHVI_STRIP_LD >= EHVI_MAX_FRONT + 2, "a_0 .. a_{n+1} at the cap");
    const int64_t LDS[4] = {2, 3, 66, EHVI_STRIP_LD};
    for (int64_t ld : LDS) {
        const long long l = (long long)ld;
        const EhviBatchWs z = ehvi_batch_ws(WsCarver(nullptr), ld);
        const int64_t total = z.bytes;
        CHECK(!z.a && !z.b && !z.y && !z.nfront && !z.n, "ld %lld: a sizing walk returned a pointer", l);
        std::vector<WsRegion> regs;
        char* base = static_cast<char*>(aligned_alloc(4096, (size_t)((total + 4095) / 4096 * 4096)));
        const EhviBatchWs w = ehvi_batch_ws(WsCarver(base, &regs), ld);
        CHECK(w.bytes == total, "ld %lld: sizing walk %lld, carving walk %lld", l, (long long)total, (long long)w.bytes);
        CHECK(reinterpret_cast<char*>(w.a) == base && w.b == w.a + ld && w.y == w.b + ld, "ld %lld: a / b / sel_y are not where the kernels read them", l);
        CHECK(reinterpret_cast<char*>(w.nfront) == reinterpret_cast<char*>(w.y + 128) && reinterpret_cast<char*>(w.n) == reinterpret_cast<char*>(w.nfront + 64),
              "ld %lld: sel_nfront / n", l);
        CHECK(total == (2 * ld + 128 + 64 + 1) * 8, "ld %lld: total %lld", l, (long long)total);
        free(base);
        CHECK(regs.size() == 5, "ld %lld: %zu regions", l, regs.size());
        int64_t end = 0;
        for (const WsRegion& r : regs) {
            CHECK(r.offset == end && r.offset % 8 == 0 && r.bytes > 0 && r.offset + r.bytes <= total, "ld %lld %s: not packed in walk order", l, r.name);
            end = r.offset + r.bytes;
        }
        for (const WsRegion& r : regs) printf("layout ehvi_batch ld%lld %s %lld %lld\n", l, r.name, (long long)r.offset, (long long)r.bytes);
        printf("layout ehvi_batch ld%lld total 0 %lld\n", l, (long long)total);
        ++nlayouts;
    }
    printf("layouts %d\n", nlayouts);
    if (bad) return 1;
    printf("ws layout ok\n");
    return 0;
}
