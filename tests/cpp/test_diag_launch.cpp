// The diagonal plan's launch resolver (spec_viterbi_amd/csrc/diag_launch.cpp) under AddressSanitizer +
// UBSan: a stand-alone host program, no HIP.
//   * tests/golden/diag_launch_grid.jsonl: what the launch code before the resolver -- diag_waves_for,
//     diag_sm_for, diag_loader_for, diag_quad_for, diag_lds_bytes and launch_diag's own grid, LDS and
//     even-placement arithmetic -- gave for each cell, recorded from that code; diag_resolve must give
//     the same, field by field.
//   * the invariants the launch and the kernels rely on, by brute force over the whole grid the golden
//     cells were picked from.
// usage: test_diag_launch tests/golden/diag_launch_grid.jsonl
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "diag_launch.h"

using namespace svh;

static int failures = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            if (failures < 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

struct Geometry {
    uint32_t nrng, nrng2, P;
    bool dtab2, dtab4;
};
// 2405.chmm's is the third; then the same without the plane table, and without the quad table
static const Geometry kGeometries[] = {
    {2, 1, 128, true, true}, {5, 3, 384, true, true}, {38, 19, 2432, true, true}, {38, 19, 2432, false, false}, {38, 19, 2432, true, false}};
static const uint32_t kS[] = {4, 20, 21, 32};
static const uint32_t kCus[] = {0, 256};
static const uint64_t kNseq[] = {1, 2, 3, 4, 5, 13, 26, 27, 50, 52, 53, 100, 400};

static DiagCaps caps_of(uint32_t S, const Geometry& g, bool sx, uint32_t cus, uint32_t dsm, uint32_t dld, uint32_t dqd) {
    DiagCaps c;
    c.S = S;
    c.P = g.P;
    c.nrng = g.nrng;
    c.nrng2 = g.dtab2 ? g.nrng2 : 0;
    c.sx = sx;
    c.cus = cus;
    c.dtab2 = g.dtab2;
    c.dtab4 = g.dtab4;
    c.ties_heavy = true;
    c.SM = 2;
    c.dsm = dsm;
    c.dld = dld;
    c.dqd = dqd;
    return c;
}

static void check_cell(const DiagCaps& c, const DiagQuery& q) {
    const DiagLaunch L = diag_resolve(c, q);
    if (L.quad) CHECK(L.loader && L.dm == 2 && c.dtab4);
    if (L.loader) CHECK(!q.paths);
    if (L.dm == 2) CHECK(c.dtab2 && !q.paths);
    CHECK(L.dm == 1 || L.dm == 2);
    CHECK(L.W == 1 || L.W == 2 || L.W == 4);
    CHECK(L.W <= kDiagMaxWaves && (L.W == 1 || L.W <= q.nseq));
    CHECK(L.floor == (L.floor && q.floor && L.loader && !L.quad && L.W == 4));
    if (q.floor) CHECK(L.ok == (L.ok && L.floor));
    CHECK(L.ranges == (L.dm == 2 ? c.nrng2 : c.nrng));
    CHECK(L.threads == 64 * (L.W + (L.loader ? 1 : 0)));
    CHECK(L.grid == (q.nseq + L.W - 1) / L.W * L.ranges);
    if (L.ok) {
        CHECK(L.lds_bytes <= kDiagLdsMax);
        CHECK(L.lds_bytes <= L.lds_request && L.lds_request <= kDiagLdsMax);
        CHECK(L.lds_bytes >= (q.paths ? diag_lds_paths(c.dk, L.W, c.S, c.sx) : (2 * (size_t)c.P + 2 * L.W) * 4));
        if (L.lds_request > L.lds_bytes) CHECK(c.cus && (L.grid + c.cus - 1) / c.cus * L.lds_request <= kDiagLdsMax);
    }
    if (!c.cus) CHECK(L.lds_request == L.lds_bytes);
    // a diagnostic build, and a build with blocks of 32 steps: the plain variant only / no quad ring, no paths
    DiagCaps d = c;
    d.variants = false;
    const DiagLaunch D = diag_resolve(d, q);
    CHECK(D.dm == 1 && !D.loader && !D.quad && !D.floor && D.threads == 64 * D.W && D.ok == (!q.paths && !q.floor));
    d = c;
    d.dk = 32;
    const DiagLaunch K = diag_resolve(d, q);
    CHECK(!K.quad && (!q.paths || !K.ok));
}

static uint64_t check_invariants() {
    uint64_t cells = 0;
    for (uint32_t S : kS)
        for (const Geometry& g : kGeometries)
            for (int sx = 0; sx < 2; ++sx)
                for (uint32_t cus : kCus)
                    for (uint32_t ov = 0; ov < 27; ++ov)
                        for (uint64_t nseq : kNseq)
                            for (int f = 0; f < 8; ++f) {
                                check_cell(caps_of(S, g, sx, cus, ov % 3, ov / 3 % 3, ov / 9), {nseq, (f & 1) != 0, (f & 2) != 0, (f & 4) != 0});
                                ++cells;
                            }
    // models the kernels do not take
    DiagCaps c = caps_of(20, kGeometries[2], false, 256, 0, 0, 0);
    CHECK(diag_resolve(c, {13}).ok);
    for (int k = 0; k < 6; ++k) {
        DiagCaps b = c;
        if (k == 0) b.S = kDiagMaxSym + 1;
        if (k == 1) b.S = 0;
        if (k == 2) b.SM = 4;
        if (k == 3) b.wide = true;
        if (k == 4) b.nrng = 0;
        if (k == 5) b.P = 64 * b.nrng - 64;
        CHECK(!diag_model_ok(b) && !diag_resolve(b, {13}).ok);
    }
    c.ties_heavy = false;
    CHECK(diag_resolve(c, {13}).ok && !diag_resolve(c, {13, false, true}).ok);
    // no sequences: nothing to launch, nothing divided by
    CHECK(diag_resolve(c, {0}).grid == 0 && diag_resolve(c, {0}).W == 1 && !diag_resolve(c, {0}).loader);
    CHECK(even_placement_lds(0, 256, 1000) == 1000 && even_placement_lds(10, 0, 1000) == 1000);
    // the named cases of DESIGN.md 5l on 2405.chmm's geometry, 256 CUs
    c = caps_of(20, kGeometries[2], false, 256, 0, 0, 0);
    CHECK(diag_resolve(c, {13}).dm == 1 && diag_resolve(c, {13}).loader && !diag_resolve(c, {13}).quad);
    CHECK(diag_resolve(c, {24}).dm == 1 && diag_resolve(c, {24}).grid == 6 * 38);  // 24 x 38 = 912 waves <= 4 x 256
    CHECK(diag_resolve(c, {25}).dm == 2 && diag_resolve(c, {25}).quad);             // 28 x 38 = 1064
    CHECK(diag_resolve(c, {50}).dm == 2 && diag_resolve(c, {50}).loader && diag_resolve(c, {50}).quad && diag_resolve(c, {50}).grid == 13 * 19);
    CHECK(diag_resolve(c, {53}).dm == 2 && !diag_resolve(c, {53}).loader && diag_resolve(c, {53}).threads == 256);  // 14 x 19 = 266 workgroups > 256
    CHECK(diag_resolve(c, {50, true}).dm == 1 && !diag_resolve(c, {50, true}).quad);
    CHECK(diag_resolve(c, {13, false, false, true}).floor && !diag_resolve(c, {3, false, false, true}).ok);
    return cells;
}

static const char* kFields[] = {"S", "P", "nrng", "nrng2", "sx", "cus", "dtab2", "dtab4", "dsm", "dld", "dqd", "nseq", "resumed",
                                "paths", "floor", "ok", "W", "dm", "loader", "quad", "is_floor", "ranges", "grid", "threads",
                                "lds_bytes", "lds_request"};
constexpr size_t kNF = sizeof(kFields) / sizeof(kFields[0]);

static uint64_t check_golden(const char* path) {
    std::FILE* f = std::fopen(path, "r");
    if (!f) {
        std::printf("FAIL cannot open %s\n", path);
        ++failures;
        return 0;
    }
    char line[1024];
    uint64_t rows = 0, lineno = 0;
    while (std::fgets(line, sizeof line, f)) {
        ++lineno;
        if (lineno == 1) {  // {"fields": [...]}: the order this program reads
            const char* at = line;
            for (size_t k = 0; k < kNF && at; ++k) {
                char quoted[40];
                std::snprintf(quoted, sizeof quoted, "\"%s\"", kFields[k]);
                at = std::strstr(at, quoted);
                if (at) at += std::strlen(quoted);
            }
            CHECK(at != nullptr);
            continue;
        }
        std::vector<uint64_t> v;
        for (const char* p = line; *p;) {
            if (*p >= '0' && *p <= '9') {
                char* e = nullptr;
                v.push_back(std::strtoull(p, &e, 10));
                p = e;
            } else {
                ++p;
            }
        }
        if (v.empty()) continue;
        if (v.size() != kNF) {
            std::printf("FAIL %s:%llu: %zu values\n", path, (unsigned long long)lineno, v.size());
            ++failures;
            continue;
        }
        DiagCaps c;
        c.S = (uint32_t)v[0];
        c.P = (uint32_t)v[1];
        c.nrng = (uint32_t)v[2];
        c.nrng2 = (uint32_t)v[3];
        c.sx = v[4] != 0;
        c.cus = (uint32_t)v[5];
        c.dtab2 = v[6] != 0;
        c.dtab4 = v[7] != 0;
        c.dsm = (uint32_t)v[8];
        c.dld = (uint32_t)v[9];
        c.dqd = (uint32_t)v[10];
        c.ties_heavy = true;
        c.SM = 2;
        const DiagLaunch L = diag_resolve(c, {v[11], v[12] != 0, v[13] != 0, v[14] != 0});
        const uint64_t got[] = {L.ok, L.W, L.dm, L.loader, L.quad, L.floor, L.ranges, L.grid, L.threads, L.lds_bytes, L.lds_request};
        for (size_t k = 0; k < sizeof(got) / sizeof(got[0]); ++k)
            if (got[k] != v[15 + k]) {
                if (failures < 20)
                    std::printf("FAIL %s:%llu: %s = %llu, recorded %llu\n", path, (unsigned long long)lineno, kFields[15 + k],
                                (unsigned long long)got[k], (unsigned long long)v[15 + k]);
                ++failures;
            }
        ++rows;
    }
    std::fclose(f);
    CHECK(rows >= 1000);
    return rows;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::printf("usage: %s tests/golden/diag_launch_grid.jsonl\n", argv[0]);
        return 2;
    }
    std::printf("%llu cells\n", (unsigned long long)check_invariants());
    std::printf("%llu golden rows\n", (unsigned long long)check_golden(argv[1]));
    std::printf("%d failures\n", failures);
    if (!failures) std::printf("ok\n");
    return failures ? 1 : 0;
}
