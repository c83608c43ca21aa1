// Host layout of the diagonal plan's quad table (built by `make tests`, run by tests/test_dtab4.py; no
// GPU is touched): for small chain-shaped models, PipePlan::dtab4 is the stated re-pairing of
// PipePlan::dtab2 -- entry c of symbol o is {ea[c], ea[(c + 64) % NP], eb[c], eb[(c + 64) % NP]}, float
// bits equal -- over position spaces of one range (NP = 128, where c + 64 folds onto the same range) and
// of two (NP = 256), full and with padded columns, which are +inf in all four values' own places.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "runtime.h"

namespace {

int failures = 0;
void check(bool ok, const std::string& what) {
    if (!ok) {
        std::fprintf(stderr, "FAIL: %s\n", what.c_str());
        ++failures;
    }
}

uint32_t bits(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}

// MSV shape: N = 0, M_1 .. M_L, C = L + 1
svh::HostModel chain(uint64_t L, uint64_t S, uint32_t seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> u(0.25f, 8.0f);
    const uint64_t n = L + 2;
    std::vector<uint64_t> scol{0, 1}, src, dst;
    std::vector<float> sval{0.5f, 1.5f}, prob, emis(S * n);
    for (float& e : emis) e = u(rng);
    for (uint64_t j = 1; j <= L; ++j) {
        src.push_back(0), dst.push_back(j), prob.push_back(u(rng));
        if (j < L) src.push_back(j), dst.push_back(j + 1), prob.push_back(u(rng));
        src.push_back(j), dst.push_back(0), prob.push_back(1.0f);  // (one shared weight into each heavy row)
        src.push_back(j), dst.push_back(L + 1), prob.push_back(2.0f);
    }
    src.push_back(0), dst.push_back(0), prob.push_back(0.5f);
    src.push_back(L + 1), dst.push_back(L + 1), prob.push_back(0.25f);
    return svh::build_host_model(n, S, scol.size(), scol.data(), sval.data(), emis.data(), src.size(), src.data(),
                                 dst.data(), prob.data());
}

void one(uint64_t L, uint64_t S, uint32_t want_np) {
    const std::string name = "L = " + std::to_string(L) + ", S = " + std::to_string(S);
    const svh::HostModel hm = chain(L, S, (uint32_t)(L * 31 + S));
    const svh::PipePlan p = svh::make_pipe_plan(hm);
    check(p.ok && p.nrng2 > 0 && !p.dtab2.empty(), name + ": a diagonal plan with two diagonals per lane");
    if (!p.ok || !p.nrng2) return;
    const uint32_t NP = 128 * p.nrng2;
    check(NP == want_np && NP == p.P, name + ": NP = " + std::to_string(NP));
    check(p.dtab2.size() == (size_t)S * 2 * NP, name + ": dtab2 size");
    check(p.dtab4.size() == (size_t)S * NP * 4, name + ": dtab4 size");
    if (p.dtab2.size() != (size_t)S * 2 * NP || p.dtab4.size() != (size_t)S * NP * 4) return;
    size_t bad = 0, finite = 0, padded = 0;
    for (uint32_t o = 0; o < S; ++o) {
        const float* ea = p.dtab2.data() + (size_t)o * 2 * NP;
        const float* eb = ea + NP;
        for (uint32_t c = 0; c < NP; ++c) {
            const float* q = p.dtab4.data() + ((size_t)o * NP + c) * 4;
            const uint32_t c2 = (c + 64) % NP;
            bad += bits(q[0]) != bits(ea[c]) || bits(q[1]) != bits(ea[c2]) || bits(q[2]) != bits(eb[c]) || bits(q[3]) != bits(eb[c2]);
            finite += std::isfinite(q[0]) ? 1 : 0;
            if (c >= L) {  // a padded column: +inf where it is the quad's own column and where it is the other's
                ++padded;
                bad += !(std::isinf(q[0]) && q[0] > 0 && std::isinf(q[2]) && q[2] > 0);
                const float* r = p.dtab4.data() + ((size_t)o * NP + (c + NP - 64) % NP) * 4;
                bad += !(std::isinf(r[1]) && r[1] > 0 && std::isinf(r[3]) && r[3] > 0);
            }
        }
    }
    check(bad == 0, name + ": " + std::to_string(bad) + " entries differ from the re-pairing of dtab2");
    check(finite == (size_t)S * L, name + ": every light row's ea is finite, nothing else");
    check(padded == (size_t)S * (NP - L), name + ": padded columns");
}

}  // namespace

int main() {
    one(128, 3, 128);  // one range, full: c + 64 folds onto the same range
    one(70, 5, 128);   // one range, 58 padded columns
    one(1, 2, 128);    // one light row
    one(256, 2, 256);  // two ranges, full
    one(200, 4, 256);  // two ranges, 56 padded columns
    one(129, 20, 256); // two ranges, the second nearly empty
    std::printf("%d failures\n", failures);
    if (!failures) std::printf("ok\n");
    return failures ? 1 : 0;
}
