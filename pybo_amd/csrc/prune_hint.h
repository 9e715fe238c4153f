// prune_hint.h -- the gate's decision of a selection-only sweep, carried from one sweep to the next.
// Plain C++, no HIP: tests/c/prune_hint_check.cpp compiles it with the host compiler alone.
//
// The gate (api.hip: select_topk_pruned under option "prune" = -1, with sweep_core's or ensemble_core's `gate`) spends a whole exact generation on a yes / no answer.  A sweep
// that pruned reports afterwards how well pruning paid -- its first-level survivor count against cap -- which is better evidence than the
// gate's proxy; where it paid clearly, the next sweep of the same shape on the same handle skips the gate and goes straight into the
// bound pass, exactly as "prune" = 1 does (done = 0).  The decision is re-earned from every sweep's own outcome; a stale one costs one
// sweep of what "prune" = 1 costs there (bound pass + seeds + the plain loop), after which the gate is back.
#pragma once
#include <stdint.h>

namespace gpx {

// What a carried decision is valid for: the covariance, the shape of the factor(s) and of the candidate set.  A single model: n = 1,
// nP its block rows, Np_min = Np.  An ensemble: the member count, the most block rows of any member, the fewest padded rows.
struct PruneHint {
    bool armed = false;
    int kernel_id = 0, n = 0;
    int64_t d = 0, nP = 0, Np_min = 0, M = 0, k = 0;
};

// `key`: the sweep at hand (its `armed` is not read).
inline bool prune_hint_matches(const PruneHint& hint, const PruneHint& key) {
    return hint.armed && hint.kernel_id == key.kernel_id && hint.n == key.n && hint.d == key.d && hint.nP == key.nP &&
           hint.Np_min == key.Np_min && hint.M == key.M && hint.k == key.k;
}

// Whether the sweep that just ended arms the hint for the next one: it pruned without falling back (path 2) and its first-level
// survivors stayed at or below HALF the fallback line cap = max(G, M / PRUNE_MAX_SHARE_DIV).  Like PRUNE_GATE_S2 a heuristic that only
// chooses between two correct paths.  In terms of cap, not of a share of M: at small M the seeds alone are M / 10.
inline bool prune_hint_after(int path, int64_t nsurv, int64_t cap) {
    return path == 2 && nsurv <= cap / 2;
}

}  // namespace gpx
