// The carried gate decision of selection-only sweeps (pybo_amd/csrc/prune_hint.h) on the host: what a hint matches and which sweep
// outcomes arm one.  Plain C++ with its own main; tests/test_prune_hint_host.py builds and runs it (also under the sanitizers).
#include <stdint.h>
#include <stdio.h>

#include "../../pybo_amd/csrc/prune_hint.h"

using gpx::PruneHint;
using gpx::prune_hint_after;
using gpx::prune_hint_matches;

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            printf("FAILED line %d: %s\n", __LINE__, #cond);            \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static PruneHint make_key() {
    PruneHint k;
    k.kernel_id = 1, k.n = 3, k.d = 8, k.nP = 64, k.Np_min = 8192, k.M = 1 << 20, k.k = 10;
    return k;
}

int main() {
    int cases = 0;

    // a default hint is unarmed and matches nothing, not even a key of all defaults
    {
        const PruneHint none;
        CHECK(!none.armed);
        CHECK(!prune_hint_matches(none, PruneHint()));
        CHECK(!prune_hint_matches(none, make_key()));
        printf("unarmed matches nothing\n");
        ++cases;
    }
    // an armed hint matches its own key, whatever the key's `armed` says; unarmed with every field equal it does not
    {
        PruneHint hint = make_key();
        hint.armed = true;
        PruneHint key = make_key();
        CHECK(prune_hint_matches(hint, key));
        key.armed = true;
        CHECK(prune_hint_matches(hint, key));
        hint.armed = false;
        CHECK(!prune_hint_matches(hint, key));
        printf("armed matches its own key\n");
        ++cases;
    }
    // every key field mismatching in turn, one step up and one step down
    {
        PruneHint hint = make_key();
        hint.armed = true;
        for (int field = 0; field < 7; ++field)
            for (int step = -1; step <= 1; step += 2) {
                PruneHint key = make_key();
                switch (field) {
                    case 0: key.kernel_id += step; break;
                    case 1: key.n += step; break;
                    case 2: key.d += step; break;
                    case 3: key.nP += step; break;
                    case 4: key.Np_min += step * 128; break;
                    case 5: key.M += step; break;
                    default: key.k += step; break;
                }
                CHECK(!prune_hint_matches(hint, key));
            }
        // a field beyond 32 bits: compared in full
        PruneHint big = make_key();
        big.armed = true;
        big.M = (int64_t)1 << 20;
        PruneHint key = make_key();
        key.M = ((int64_t)1 << 20) + ((int64_t)1 << 32);
        CHECK(!prune_hint_matches(big, key));
        printf("each of 7 key fields decides\n");
        ++cases;
    }
    // the rule: pruned without falling back, at most HALF the fallback line of first-level survivors
    {
        const int64_t caps[] = {4096, 10240, 10241, 262144, 1, 0};
        for (int64_t cap : caps) {
            CHECK(prune_hint_after(2, 0, cap));
            CHECK(prune_hint_after(2, cap / 2, cap));
            CHECK(!prune_hint_after(2, cap / 2 + 1, cap));
            CHECK(!prune_hint_after(2, cap + 1, cap));
        }
        CHECK(prune_hint_after(2, 5120, 10240) && !prune_hint_after(2, 5121, 10240));
        CHECK(prune_hint_after(2, 5120, 10241) && !prune_hint_after(2, 5121, 10241));      // cap / 2 rounds down
        printf("rule at cap / 2 and cap / 2 + 1\n");
        ++cases;
    }
    // no sweep yet, plain, gate declined, fell back: never, whatever the count says
    {
        const int paths[] = {-1, 0, 1, 3, 4};
        for (int path : paths) {
            CHECK(!prune_hint_after(path, 0, 10240));
            CHECK(!prune_hint_after(path, 5120, 10240));
            CHECK(!prune_hint_after(path, 20000, 10240));
        }
        printf("paths other than 2 never arm\n");
        ++cases;
    }
    if (failures) {
        printf("prune hint FAILED %d checks\n", failures);
        return 1;
    }
    printf("prune hint ok %d cases\n", cases);
    return 0;
}
