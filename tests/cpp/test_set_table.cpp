// The model sets' block table (spec_viterbi_amd/csrc/set_table.cpp) under AddressSanitizer + UBSan:
// a stand-alone host program, no HIP.  For sets of 1, 64, 65 and 200 entries, with members outside the
// set launch interleaved, every block of the grid must map to the entry and local block that a plain
// walk over the members gives; zero-range and zero-sequence members, bad workgroup widths and grids
// past 2^31 - 1 are refused.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "set_table.h"

using svh::SetMember;
using svh::SetTable;

static int failures = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static SetMember mem(uint32_t nrng, uint32_t nseq, uint32_t waves, bool grouped) {
    SetMember m;
    m.nrng = nrng;
    m.nseq = nseq;
    m.waves = waves;
    m.grouped = grouped;
    return m;
}

// every block, by brute force: walk the members in order, block by block
static void check_all_blocks(const std::vector<SetMember>& ms, const SetTable& t) {
    uint64_t bx = 0;
    uint32_t e = 0;
    for (size_t i = 0; i < ms.size(); ++i) {
        if (!ms[i].grouped) continue;
        const uint64_t blocks = ((uint64_t)ms[i].nseq + ms[i].waves - 1) / ms[i].waves * ms[i].nrng;
        CHECK(e < t.entries() && t.member[e] == i && t.first[e] == bx);
        for (uint64_t l = 0; l < blocks; ++l, ++bx) {
            uint32_t ge = ~0u, gl = ~0u;
            svh::set_table_lookup(t, (uint32_t)bx, &ge, &gl);
            if (ge != e || gl != l) {
                std::printf("FAIL block %llu: entry %u local %u, expected %u %llu\n", (unsigned long long)bx, ge, gl, e,
                            (unsigned long long)l);
                ++failures;
                return;
            }
        }
        ++e;
    }
    CHECK(e == t.entries() && bx == t.grid && t.first.size() == (size_t)e + 1 && t.first[e] == bx);
}

static void sized(uint32_t entries, uint32_t waves, uint32_t nseq, bool interleave) {
    std::vector<SetMember> ms;
    uint32_t x = 12345u + entries;
    for (uint32_t i = 0; i < entries; ++i) {
        x = x * 1664525u + 1013904223u;
        // ranges 1, 1, 2, 3, 38 ...: one-block neighbours at the boundaries
        const uint32_t nr = (x >> 24) % 5 == 0 ? 38 : 1 + (x >> 20) % 3;
        if (interleave && i % 3 == 1) ms.push_back(mem((x >> 8) % 7, nseq, waves, false));  // (zero ranges allowed: skipped)
        ms.push_back(mem(nr, nseq, waves, true));
    }
    if (interleave) ms.push_back(mem(0, 0, 0, false));
    SetTable t;
    std::string err;
    CHECK(svh::build_set_table(ms.data(), ms.size(), &t, &err));
    CHECK(t.entries() == entries);
    check_all_blocks(ms, t);
}

int main() {
    for (uint32_t entries : {1u, 2u, 63u, 64u, 65u, 128u, 129u, 200u})
        for (uint32_t waves : {1u, 2u, 4u})
            for (uint32_t nseq : {1u, 3u, 5u})
                for (bool il : {false, true}) sized(entries, waves, nseq, il);

    SetTable t;
    std::string err;
    // no grouped member: an empty table
    {
        std::vector<SetMember> ms = {mem(3, 2, 2, false), mem(0, 0, 0, false)};
        CHECK(svh::build_set_table(ms.data(), ms.size(), &t, &err) && t.entries() == 0 && t.grid == 0 && t.first.size() == 1);
        CHECK(svh::build_set_table(nullptr, 0, &t, &err) && t.entries() == 0 && t.grid == 0);
    }
    // guards: zero ranges, zero sequences, widths other than 1 / 2 / 4, null arguments
    {
        std::vector<SetMember> ms = {mem(2, 3, 2, true), mem(0, 3, 2, true)};
        CHECK(!svh::build_set_table(ms.data(), ms.size(), &t, &err) && !err.empty());
        ms[1] = mem(2, 0, 2, true);
        CHECK(!svh::build_set_table(ms.data(), ms.size(), &t, &err));
        for (uint32_t w : {0u, 3u, 5u, 8u}) {
            ms[1] = mem(2, 3, w, true);
            CHECK(!svh::build_set_table(ms.data(), ms.size(), &t, &err));
        }
        CHECK(!svh::build_set_table(ms.data(), ms.size(), nullptr, &err));
        CHECK(!svh::build_set_table(nullptr, 2, &t, nullptr));
    }
    // overflow: the largest grid that fits, one block more, one member too large on its own, a sum of
    // members that passes 2^31 - 1, factors whose product passes 2^64
    {
        std::vector<SetMember> ms = {mem(0x7FFFFFFFu, 1, 1, true)};
        CHECK(svh::build_set_table(ms.data(), ms.size(), &t, &err) && t.grid == 0x7FFFFFFFull && t.first[1] == 0x7FFFFFFFu);
        uint32_t e = 9, l = 9;
        svh::set_table_lookup(t, 0x7FFFFFFEu, &e, &l);
        CHECK(e == 0 && l == 0x7FFFFFFEu);
        ms.push_back(mem(1, 1, 1, true));
        CHECK(!svh::build_set_table(ms.data(), ms.size(), &t, &err) && err.find("grid") != std::string::npos);
        ms = {mem(0x80000000u, 1, 1, true)};
        CHECK(!svh::build_set_table(ms.data(), ms.size(), &t, &err));
        ms = {mem(0x40000000u, 4, 4, true), mem(0x3FFFFFFFu, 2, 2, true), mem(1, 1, 1, true)};
        CHECK(!svh::build_set_table(ms.data(), ms.size(), &t, &err));
        ms.pop_back();
        CHECK(svh::build_set_table(ms.data(), ms.size(), &t, &err) && t.grid == 0x7FFFFFFFull);
        ms = {mem(0xFFFFFFFFu, 0xFFFFFFFFu, 1, true), mem(0xFFFFFFFFu, 0xFFFFFFFFu, 1, true)};
        CHECK(!svh::build_set_table(ms.data(), ms.size(), &t, &err));
        ms = {mem(1000, 0xFFFFFFFFu, 4, true)};  // 2^30 groups x 1000 ranges
        CHECK(!svh::build_set_table(ms.data(), ms.size(), &t, &err));
    }
    std::printf("%d failures\n", failures);
    if (failures == 0) std::printf("ok\n");
    return failures ? 1 : 0;
}
