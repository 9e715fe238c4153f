// Host checker of pybo_amd/csrc/ws_layout.h, the one description of every device workspace (tests/test_ws_layout_host.py).
// Runs every walk over a fixed list of shapes -- the smallest at which the arithmetic can go wrong -- twice, on a null base (sizing) and
// on a real allocation of exactly that size, and prints one line per region and one per total:
//     layout <name> <shape-tag> <field> <offset> <bytes>
//     layout <name> <shape-tag> total 0 <bytes>
// which the Python side holds against tests/golden/ws_layouts.json.  Checked here, for every layout and shape: both walks give the same
// total; every region lies inside it; the regions are pairwise disjoint; the first pointer is the base (the carver itself asserts that
// every region starts on its element type's alignment); the alignments the kernels are tuned for hold (joint parts 256 bytes, the
// announcement's v 512, the bound kernels' operands 32); the announcement and the batch buffer agree on their shared front; what is
// sized by capacity holds the carving of every smaller current size.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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

struct Layout { std::vector<WsRegion> regs; int64_t total; };

static const WsRegion* find(const Layout& l, const char* name) {
    for (const WsRegion& r : l.regs)
        if (!strcmp(r.name, name)) return &r;
    return nullptr;
}

// walk: WsCarver -> the layout's struct; first: the member that must be the base
template <typename Walk, typename First>
static Layout run(const char* name, const std::string& tag, Walk walk, First first) {
    Layout l;
    l.total = walk(WsCarver(nullptr)).bytes;
    char* base = static_cast<char*>(aligned_alloc(4096, (size_t)((l.total + 4095) / 4096 * 4096 + 4096)));
    const auto w = walk(WsCarver(base, &l.regs));
    const char* t = tag.c_str();
    CHECK(w.bytes == l.total, "%s %s: sizing walk %lld, carving walk %lld", name, t, (long long)l.total, (long long)w.bytes);
    CHECK(reinterpret_cast<char*>(w.*first) == base, "%s %s: the first region is not the base", name, t);
    CHECK(walk(WsCarver(nullptr)).*first == nullptr, "%s %s: a sizing walk returned a pointer", name, t);
    free(base);
    std::vector<WsRegion> by = l.regs;
    std::sort(by.begin(), by.end(), [](const WsRegion& a, const WsRegion& b) { return a.offset < b.offset; });
    int64_t end = 0;
    for (const WsRegion& r : by) {
        CHECK(r.offset >= 0 && r.bytes >= 0 && r.offset + r.bytes <= l.total, "%s %s %s: out of bounds", name, t, r.name);
        if (r.bytes == 0) continue;
        CHECK(r.offset >= end, "%s %s %s: overlaps the region before it", name, t, r.name);
        end = r.offset + r.bytes;
    }
    for (const WsRegion& r : l.regs) printf("layout %s %s %s %lld %lld\n", name, t, r.name, (long long)r.offset, (long long)r.bytes);
    printf("layout %s %s total 0 %lld\n", name, t, (long long)l.total);
    ++nlayouts;
    return l;
}

static void aligned(const Layout& l, const char* what, const std::string& tag, std::initializer_list<const char*> names, int64_t to) {
    for (const char* n : names) {
        const WsRegion* r = find(l, n);
        if (r) CHECK(r->offset % to == 0, "%s %s %s: offset %lld is not a multiple of %lld", what, tag.c_str(), n, (long long)r->offset, (long long)to);
    }
}

static std::string tagf(const char* fmt, long long a = 0, long long b = 0, long long c = 0, long long d = 0, long long e = 0, long long f = 0) {
    char buf[160];
    snprintf(buf, sizeof buf, fmt, a, b, c, d, e, f);
    return buf;
}

// the bound kernel's k-steps for dimension d (kernels_sweep.hip: bound_mfma_normc / bound_mfma_steps)
static bool normc(int d) { return d > 0 && (d + 3) / 4 < (d + 5) / 4; }
static int steps(int d) { return normc(d) ? (d + 3) / 4 : (d + 5) / 4; }

int main() {
    const int64_t NPS[3] = {128, 1024, 1152};
    const int64_t MS[5] = {1, 127, 1000, 4096, 32768};
    const int DS[5] = {1, 3, 8, 18, 19};

    for (int i = 0; i < 5; ++i)
        for (int withx = 0; withx < 2; ++withx) {
            const int64_t M = MS[i], nx = withx ? M * DS[i] : 0;
            run("staged", tagf("d%lld_M%lld_x%lld", DS[i], M, withx), [&](WsCarver c) { return staged_ws(c, nx, M); }, &StagedWs::X);
        }
    for (int64_t M : MS) run("ens", tagf("M%lld", M), [&](WsCarver c) { return ens_ws(c, M); }, &EnsWs::acc0);

    // the bound kernels' operands: one size for every d, every operand on 32 bytes
    for (int64_t Np : NPS) {
        int64_t total = -1;
        for (int d = 1; d <= 18; ++d) {
            struct Ops : BoundOps { int64_t bytes; };
            const Layout l = run("bound_ops", tagf("Np%lld_d%lld", Np, d), [&](WsCarver c) {
                Ops o;
                static_cast<BoundOps&>(o) = bound_ops(c, Np, steps(d), normc(d));
                o.bytes = c.bytes();
                return o;
            }, &Ops::A);
            aligned(l, "bound_ops", tagf("Np%lld_d%lld", Np, d), {"A", "W4", "NX4", "cen", "A32", "W32", "WF32", "NX32"}, 32);
            CHECK(total < 0 || total == l.total, "bound_ops Np %lld d %d: the size depends on d", (long long)Np, d);
            total = l.total;
        }
    }

    // the pruning workspace: the geometry of api.hip's prune_geom (G a generation of at least k, Gg a full one, cap >= G)
    int nprune = 0;
    for (int di = 0; di < 5; ++di)
        for (int mi = 0; mi < 5; ++mi) {
            const int64_t d = DS[di], M = MS[mi], Np = NPS[(di + mi) % 3], k = (di + mi) % 2 ? 4096 : 1, nP = Np / NB;
            const int64_t gen = std::max<int64_t>(1, 512 / ((nP + 1) / 2));
            const int64_t G = std::max<int64_t>((int64_t)TBH * std::min<int64_t>(32, gen), (k + TBH - 1) / TBH * TBH);
            const int64_t Gg = (int64_t)TBH * gen, cap = std::max<int64_t>(G, M / 4);
            for (int rows = 0; rows < 2; ++rows) {
                if ((di + mi + rows) % 2) continue;       // (half of the grid: every d, M, Np, k and both forms still occur)
                const int64_t extra = rows ? 0 : 3 * 5;      // the ensemble lead's words, five members
                const std::string tag = tagf("d%lld_Np%lld_M%lld_k%lld_rows%lld_x%lld", d, Np, M, k, rows, extra);
                const Layout l = run("prune", tag, [&](WsCarver c) { return prune_ws_layout(c, M, cap, d, Np, Gg, extra, rows != 0); }, &PruneWs::ub);
                aligned(l, "prune", tag, {"A", "W4", "cen", "A32", "W32", "WF32"}, 32);
                ++nprune;
            }
        }
    // a member of an ensemble sweep: nothing but the bound pass's part
    run("prune", "member_d8_Np1024", [&](WsCarver c) { return prune_ws_layout(c, 0, 0, 8, 1024, 0, 0, false); }, &PruneWs::ub);
    CHECK(nprune >= 12, "prune: %d shapes", nprune);

    const int64_t KEEP[3][2] = {{1, 128}, {127, 4096}, {32768, 4096}};
    for (auto& s : KEEP) run("keep", tagf("M%lld_G%lld", s[0], s[1]), [&](WsCarver c) { return keep_ws(c, s[0], s[1]); }, &KeepWs::ub);
    for (int64_t ld : NPS) run("pend", tagf("ld%lld", ld), [&](WsCarver c) { return pend_ws(c, ld); }, &PendWs::rows);

    // gpx_append's scratch and predict-with-gradients: sized at the capacity, carved at the current size
    const int64_t APP[4][3] = {{1, 128, 128}, {19, 1024, 1152}, {65, 1152, 1152}, {8, 1024, 1024}};      // d, Np, cap_np
    for (auto& s : APP) {
        const int64_t xpad = (s[0] + 63) / 64 * 64;
        const Layout cur = run("append", tagf("d%lld_Np%lld", s[0], s[1]), [&](WsCarver c) { return append_ws(c, xpad, s[1]); }, &AppendWs::x);
        CHECK(cur.total <= append_ws(WsCarver(nullptr), xpad, s[2]).bytes, "append: the capacity's size does not hold the carving");
        const int64_t nseg = (s[1] + 1023) / 1024, nseg_cap = (s[2] + 1023) / 1024;
        const Layout g = run("grad", tagf("d%lld_Np%lld_nseg%lld", s[0], s[1], nseg), [&](WsCarver c) { return grad_ws(c, s[0], s[1], nseg); }, &GradWs::X);
        CHECK(g.total <= grad_ws(WsCarver(nullptr), s[0], s[2], nseg_cap).bytes, "grad: the capacity's size does not hold the carving");
    }
    const int64_t RG[3][3] = {{1, 1, 1}, {5, 3, 127}, {128, 19, 5}};      // n, d, M
    for (auto& s : RG) run("rff_grad", tagf("n%lld_d%lld_M%lld", s[0], s[1], s[2]), [&](WsCarver c) { return rff_grad_ws(c, s[0], s[1], s[2]); }, &RffGradWs::W);

    // the announcement and the batch buffer: v on 512 bytes, one front
    const int64_t SPEC[5][5] = {{8, 1024, 1000, 4, 0}, {1, 128, 1, 1, 0}, {19, 1152, 127, 64, 5}, {3, 1024, 32768, 2, 1}, {18, 1024, 4096, 1, 0}};   // cap_d, cap_np, M, nb, n_lead
    for (auto& s : SPEC) {
        const int64_t xpad = (s[0] + 63) / 64 * 64, M = s[2], nb = s[3], nl = s[4];
        for (int64_t ld : {s[1], s[1] + NB}) {
            const std::string tag = tagf("d%lld_ld%lld_M%lld", s[0], ld, M);
            const Layout sp = run("spec", tag, [&](WsCarver c) { return spec_ws(c, xpad, ld, M); }, &SpecBuf::x);
            aligned(sp, "spec", tag, {"v"}, 512);
            const std::string btag = tagf("d%lld_ld%lld_M%lld_nb%lld_lead%lld", s[0], ld, M, nb, nl);
            const Layout ba = run("batch", btag, [&](WsCarver c) { return batch_ws(c, xpad, ld, M, nb, nl, (nl * 88 + 7) / 8); }, &BatchBuf::x);
            for (const char* f : {"x", "xs", "ks", "g", "r", "tu", "row"}) {
                const WsRegion *a = find(sp, f), *b = find(ba, f);
                CHECK(a && b && a->offset == b->offset && a->bytes == b->bytes, "spec / batch %s: the fronts differ at %s", tag.c_str(), f);
            }
            const WsRegion *row = find(ba, "row"), *pv = find(ba, "partv");
            CHECK(row && pv && pv->offset == row->offset + row->bytes + 384 * 8, "batch %s: the small state is not 384 doubles", btag.c_str());
        }
    }

    const int64_t JOINT[5][5] = {{1, 1, 128, 0, 0}, {127, 3, 1024, 1, 1}, {1000, 19, 1152, 1, 5}, {129, 8, 1024, 0, 0}, {5, 18, 128, 1, 5}};   // M, d, Np, draw, S
    for (auto& s : JOINT) {
        const int64_t M = s[0], Mp = (M + TBH - 1) / TBH * TBH;
        const std::string tag = tagf("M%lld_d%lld_Np%lld_draw%lld_S%lld", M, s[1], s[2], s[3], s[4]);
        const Layout l = run("joint", tag, [&](WsCarver c) { return joint_ws(c, M, Mp, s[1], s[2] / NB, s[2], s[3] != 0, s[4]); }, &JointWs::X);
        aligned(l, "joint", tag, {"X", "Zs", "mu", "Pp", "V", "Kss", "C", "B", "R", "z"}, 256);
    }
    const int64_t KG[3][3] = {{1, 1, 128}, {127, 18, 1024}, {1000, 19, 1152}};      // M, d, Np
    for (auto& s : KG) {
        run("kg", tagf("d%lld_Np%lld", s[1], s[2]), [&](WsCarver c) { return kg_ws(c, s[1], s[2], 1); }, &KgBuf::A);
        const int64_t Mp = (s[0] + TBH - 1) / TBH * TBH;
        run("kg_point", tagf("M%lld_d%lld_Np%lld", s[0], s[1], s[2]), [&](WsCarver c) { return kg_point_ws(c, Mp, s[1], s[2]); }, &KgPointWs::Z);
    }

    const int64_t RFF[4][4] = {{1, 1, 1, 128}, {5, 5, 3, 1024}, {5, 127, 19, 1152}, {1, 257, 8, 1024}};      // S, n, d, Np
    for (auto& s : RFF) {
        const int64_t S = s[0], n = s[1], d = s[2], Np = s[3], dp = (d + 3) / 4 * 4, nfb = (n + TBH - 1) / TBH;
        const std::string tag = tagf("S%lld_n%lld_d%lld_Np%lld", S, n, d, Np);
        run("rff_sweep", tag, [&](WsCarver c) { return rff_sweep_ws(c, S * nfb * dp * TBH, S * nfb * TBH); }, &RffSweepWs::Wt);
        if (n < TBH)
            for (int64_t extra : {(int64_t)0, 2 * S * n})
                run("rff_gram", tag + tagf("_x%lld", extra), [&](WsCarver c) { return rff_gram_ws(c, S * dp * TBH, S * TBH, S, n, extra); }, &RffGramWs::Wt);
        const int64_t nw = std::max<int64_t>(n, TBH), np = (nw + NB - 1) / NB * NB;
        for (int post = 0; post < 2; ++post)
            run("rff_wide", tagf("n%lld_d%lld_Np%lld_post%lld", nw, d, Np, post), [&](WsCarver c) { return rff_wide_ws(c, nw, d, post ? np : 0, Np, post != 0); }, &RffWideWs::W);
    }

    const int64_t LB[5][3] = {{1, 128, 1}, {2, 128, 3}, {5, 1024, 19}, {64, 128, 8}, {5, 128, 18}};      // B, Np, d
    for (auto& s : LB) {
        const std::string tag = tagf("B%lld_Np%lld_d%lld", s[0], s[1], s[2]);
        const Layout l = run("loglik_batch", tag, [&](WsCarver c) { return loglik_batch_ws(c, s[0], s[1], s[2]); }, &LoglikBatchWs::S);
        CHECK(l.total % 8 == 0, "loglik_batch %s: the size is not whole doubles", tag.c_str());
    }
    const int64_t HY[4][3] = {{1, 1, 1}, {8, 19, 9}, {9, 8, 9}, {9, 19, 9}};      // nP, d, the capacity's block rows
    for (auto& s : HY) {
        const Layout l = run("hyper", tagf("nP%lld_d%lld", s[0], s[1]), [&](WsCarver c) { return hyper_ws(c, s[0] * (s[0] + 1) / 2, s[1]); }, &HyperWs::part);
        CHECK(l.total <= hyper_ws(WsCarver(nullptr), s[2] * (s[2] + 1) / 2, 19).bytes, "hyper: the capacity's size does not hold the carving");
    }

    printf("layouts %d\n", nlayouts);
    if (bad) {
        printf("ws layout FAILED: %d checks\n", bad);
        return 1;
    }
    printf("ws layout ok\n");
    return 0;
}
