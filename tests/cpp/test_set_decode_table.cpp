// The block tables of a model set's decode pass (spec_viterbi_amd/csrc/set_table.cpp) under
// AddressSanitizer + UBSan: a stand-alone host program, no HIP.  A decode's members differ in their row
// counts -- the chosen rows of each model -- so entry e of the forward table covers ceil(rows / W) x
// ranges blocks and entry e of the traceback table (build_set_row_table) one block per row.  For row
// counts 0 (the member is in neither table), 1, W - 1, W and W + 1 at every workgroup width, in sets of
// up to 65 entries, every block of both grids must map to the entry and the local block (forward) or the
// row (traceback) that a plain walk over the members gives; grids past kSetMaxGrid are refused.
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

static SetMember mem(uint32_t nrng, uint32_t rows, uint32_t waves) {
    SetMember m;
    m.nrng = nrng;
    m.nseq = rows;
    m.waves = waves;
    m.grouped = rows != 0;  // a member without chosen rows runs nothing
    return m;
}

// every block of a table, by brute force; blocks(m) = the blocks a member has in it
template <class Blocks>
static void check_all_blocks(const char* what, const std::vector<SetMember>& ms, const SetTable& t, Blocks blocks) {
    uint64_t bx = 0;
    uint32_t e = 0;
    for (size_t i = 0; i < ms.size(); ++i) {
        if (!ms[i].grouped) continue;
        CHECK(e < t.entries() && t.member[e] == i && t.first[e] == bx);
        const uint64_t nb = blocks(ms[i]);
        for (uint64_t l = 0; l < nb; ++l, ++bx) {
            uint32_t ge = ~0u, gl = ~0u;
            svh::set_table_lookup(t, (uint32_t)bx, &ge, &gl);
            if (ge != e || gl != l) {
                std::printf("FAIL %s block %llu: entry %u local %u, expected %u %llu\n", what, (unsigned long long)bx, ge, gl, e,
                            (unsigned long long)l);
                ++failures;
                return;
            }
        }
        ++e;
    }
    CHECK(e == t.entries() && bx == t.grid && t.first.size() == (size_t)e + 1 && t.first[e] == bx);
}

static void sized(uint32_t members, uint32_t W, uint32_t shift) {
    const uint32_t rows[5] = {0, 1, W - 1, W, W + 1};  // (W = 1: 0 twice)
    std::vector<SetMember> ms;
    uint32_t x = 777u + members * 31u + W, present = 0;
    for (uint32_t i = 0; i < members; ++i) {
        x = x * 1664525u + 1013904223u;
        const uint32_t nr = (x >> 24) % 7 == 0 ? 38 : 1 + (x >> 20) % 3;
        ms.push_back(mem(nr, rows[(i + shift) % 5], W));
        present += ms.back().grouped ? 1u : 0u;
    }
    SetTable fwd, tb;
    std::string err;
    CHECK(svh::build_set_table(ms.data(), ms.size(), &fwd, &err));
    CHECK(svh::build_set_row_table(ms.data(), ms.size(), &tb, &err));
    CHECK(fwd.entries() == present && tb.entries() == present && fwd.member == tb.member);
    check_all_blocks("forward", ms, fwd, [](const SetMember& m) { return ((uint64_t)m.nseq + m.waves - 1) / m.waves * m.nrng; });
    check_all_blocks("traceback", ms, tb, [](const SetMember& m) { return (uint64_t)m.nseq; });
    uint64_t nrows = 0;
    for (const SetMember& m : ms) nrows += m.grouped ? m.nseq : 0;
    CHECK(tb.grid == nrows);
}

int main() {
    // (82 members: 65 entries at W >= 2, where one row count in five is 0)
    for (uint32_t members : {1u, 5u, 64u, 65u, 80u, 82u})
        for (uint32_t W : {1u, 2u, 4u})
            for (uint32_t shift : {0u, 1u, 2u, 3u, 4u}) sized(members, W, shift);
    {
        std::vector<SetMember> ms;
        for (uint32_t i = 0; i < 82; ++i) ms.push_back(mem(1 + i % 3, i % 5 == 0 ? 0 : 1 + i % 6, 4));
        SetTable t;
        CHECK(svh::build_set_row_table(ms.data(), ms.size(), &t) && t.entries() == 65);
    }

    SetTable t;
    std::string err;
    // no member with rows: empty tables
    {
        std::vector<SetMember> ms = {mem(3, 0, 2), mem(1, 0, 4)};
        CHECK(svh::build_set_table(ms.data(), ms.size(), &t, &err) && t.entries() == 0 && t.grid == 0);
        CHECK(svh::build_set_row_table(ms.data(), ms.size(), &t, &err) && t.entries() == 0 && t.grid == 0 && t.first.size() == 1);
        CHECK(svh::build_set_row_table(nullptr, 0, &t, &err) && t.entries() == 0);
    }
    // the row table takes a member for its rows alone; null arguments are refused
    {
        std::vector<SetMember> ms = {mem(38, 5, 4), mem(2, 3, 2)};
        CHECK(svh::build_set_row_table(ms.data(), ms.size(), &t, &err) && t.grid == 8 && t.first[1] == 5);
        CHECK(!svh::build_set_row_table(ms.data(), ms.size(), nullptr, &err));
        CHECK(!svh::build_set_row_table(nullptr, 2, &t, &err) && !err.empty());
    }
    // grids past kSetMaxGrid: the forward table of rows x ranges, the row table of rows alone
    {
        std::vector<SetMember> ms = {mem(2, 0x7FFFFFFFu, 1)};
        CHECK(!svh::build_set_table(ms.data(), ms.size(), &t, &err) && err.find("grid") != std::string::npos);
        CHECK(svh::build_set_row_table(ms.data(), ms.size(), &t, &err) && t.grid == svh::kSetMaxGrid);
        uint32_t e = 9, l = 9;
        svh::set_table_lookup(t, 0x7FFFFFFEu, &e, &l);
        CHECK(e == 0 && l == 0x7FFFFFFEu);
        ms.push_back(mem(1, 1, 1));
        CHECK(!svh::build_set_row_table(ms.data(), ms.size(), &t, &err) && err.find("grid") != std::string::npos);
        ms = {mem(1, 0x80000000u, 4)};  // 2^29 forward blocks, 2^31 rows
        CHECK(svh::build_set_table(ms.data(), ms.size(), &t, &err));
        CHECK(!svh::build_set_row_table(ms.data(), ms.size(), &t, &err));
    }
    std::printf("%d failures\n", failures);
    if (failures == 0) std::printf("ok\n");
    return failures ? 1 : 0;
}
