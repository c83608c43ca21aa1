// The chain planner on MSV-shaped models whose N and C sit at any state index (built by `make tests`,
// run by tests/test_chain_place_cases.py; no GPU is touched): with and without the M -> N terms --
// without them N's in-degree is 1, so only its place in the chain rule tells band_heavy_rows
// (runtime.cpp) that it is a heavy row -- every chain, band and pipelined plan is built, F and S are
// N and C, the positions are the light rows in chain order, and F wins every tie exactly where N lies
// below every light row.
#include <cstdio>
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

// N at state n_at, C at c_at, the light rows at the other indices in chain order
svh::HostModel placed_chain(uint64_t L, uint64_t n_at, uint64_t c_at, bool m_to_n) {
    const uint64_t n = L + 2, S = 3;
    std::vector<uint64_t> m, scol{n_at}, src, dst;  // m[j - 1]: state of M_j
    std::vector<float> sval{0.0f}, prob, emis(S * n, 1.0f);
    for (uint64_t s = 0; s < n; ++s)
        if (s != n_at && s != c_at) m.push_back(s);
    for (uint64_t j = 0; j < L; ++j) {
        src.push_back(n_at), dst.push_back(m[j]), prob.push_back(1.0f + (float)(j % 3));
        if (j + 1 < L) src.push_back(m[j]), dst.push_back(m[j + 1]), prob.push_back(2.0f);
        if (m_to_n) src.push_back(m[j]), dst.push_back(n_at), prob.push_back(3.0f);
        src.push_back(m[j]), dst.push_back(c_at), prob.push_back(1.0f);
    }
    src.push_back(n_at), dst.push_back(n_at), prob.push_back(0.5f);
    src.push_back(c_at), dst.push_back(c_at), prob.push_back(0.25f);
    return svh::build_host_model(n, S, scol.size(), scol.data(), sval.data(), emis.data(), src.size(), src.data(),
                                 dst.data(), prob.data());
}

void one(uint64_t L, uint64_t n_at, uint64_t c_at, bool m_to_n) {
    const std::string name = "L=" + std::to_string(L) + " N=" + std::to_string(n_at) + " C=" + std::to_string(c_at) +
                             (m_to_n ? "" : " without M -> N");
    const svh::HostModel hm = placed_chain(L, n_at, c_at, m_to_n);
    for (bool chain : {true, false}) {
        const svh::BandPlan b = svh::make_band_plan(hm, 0, chain);
        check(b.ok && b.HA == 1 && b.H == 2 && b.nL == L, name + (chain ? ": chain plan" : ": band plan"));
        if (b.ok) check(b.hrow[0] == (int)n_at && b.hrow[1] == (int)c_at, name + ": heavy rows of the band plan");
    }
    const uint64_t first_light = n_at != 0 && c_at != 0 ? 0 : n_at != 1 && c_at != 1 ? 1 : 2;
    for (bool wide : {false, true}) {
        const svh::PipePlan p = svh::make_pipe_plan(hm, 0, 0, wide);
        check(p.ok && p.rowF == (int)n_at && p.rowS == (int)c_at, name + ": pipelined plan, F and S");
        if (!p.ok) continue;
        uint32_t next = 0;
        bool rows = p.lrow.size() == p.P && p.P >= L;
        for (uint32_t pos = 0; rows && pos < p.P; ++pos) {
            while (next == n_at || next == c_at) ++next;
            rows = pos < L ? p.lrow[pos] == next++ : p.lrow[pos] == 0xFFFFFFFFu;
        }
        check(rows, name + ": positions in chain order, padding past them");
        check(p.ties_heavy == (n_at < first_light), name + ": ties_heavy");
        check(p.spos[n_at] == -1 && p.spos[c_at] == -2, name + ": state -> position map of the heavy rows");
    }
}

}  // namespace

int main() {
    int models = 0;
    for (uint64_t L : {3, 70, 300})
        for (bool m_to_n : {true, false}) {
            const uint64_t places[6][2] = {{0, L + 1}, {L + 1, 0}, {1, 0}, {L + 1, L}, {L / 2, L / 2 + 1}, {0, L / 2 + 1}};
            for (const auto& pl : places) {
                one(L, pl[0], pl[1], m_to_n);
                ++models;
            }
        }
    std::printf("%d models, %d failures\n", models, failures);
    if (!failures) std::printf("ok\n");
    return failures ? 1 : 0;
}
