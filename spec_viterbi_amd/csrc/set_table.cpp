#include "set_table.h"

namespace svh {

bool build_set_table(const SetMember* members, uint64_t count, SetTable* out, std::string* err) {
    auto fail = [&](const std::string& what) {
        if (err) *err = what;
        return false;
    };
    if (!out || (count && !members)) return fail("null argument");
    if (count > 0xFFFFFFFFull) return fail("too many members");
    out->first.assign(1, 0u);
    out->member.clear();
    out->grid = 0;
    uint64_t at = 0;
    for (uint64_t i = 0; i < count; ++i) {
        const SetMember& m = members[i];
        if (!m.grouped) continue;
        if (m.nrng == 0 || m.nseq == 0) return fail("member " + std::to_string(i) + ": a grouped member without ranges or sequences");
        if (m.waves != 1 && m.waves != 2 && m.waves != 4)
            return fail("member " + std::to_string(i) + ": workgroups of 1, 2 or 4 sequences");
        const uint64_t groups = ((uint64_t)m.nseq + m.waves - 1) / m.waves;
        const uint64_t blocks = groups * m.nrng;  // (< 2^64: both factors are below 2^32)
        if (blocks > kSetMaxGrid || at + blocks > kSetMaxGrid) return fail("the set's grid exceeds 2^31 - 1 workgroups");
        at += blocks;
        out->member.push_back((uint32_t)i);
        out->first.push_back((uint32_t)at);
    }
    out->grid = at;
    return true;
}

bool build_set_row_table(const SetMember* members, uint64_t count, SetTable* out, std::string* err) {
    if (count && !members) {
        if (err) *err = "null argument";
        return false;
    }
    std::vector<SetMember> rows(members, members + count);
    for (SetMember& m : rows)
        if (m.grouped) m.nrng = 1, m.waves = 1;  // a block per sequence
    return build_set_table(rows.data(), count, out, err);
}

void set_table_lookup(const SetTable& t, uint32_t bx, uint32_t* entry, uint32_t* local) {
    const uint32_t ne = t.entries();
    uint32_t cnt = 0;
    for (uint32_t i0 = 0; i0 < ne; i0 += 64) {
        uint32_t c = 0;
        for (uint32_t l = 0; l < 64; ++l) c += (i0 + l < ne && t.first[i0 + l] <= bx) ? 1u : 0u;
        cnt += c;
        if (c < 64) break;
    }
    *entry = cnt - 1;
    *local = bx - t.first[cnt - 1];
}

}  // namespace svh
