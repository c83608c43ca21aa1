// Block table of a model-set launch (diag.hip diag_set_kernel; runtime.cpp BatchSet): plain host
// code, no HIP.  The grid of a set launch is the concatenation of its grouped members' own grids;
// entry e covers blocks [first[e], first[e + 1]) and belongs to member member[e].
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace svh {

struct SetMember {
    uint32_t nrng = 0;     // ranges of 64 diagonals per sequence
    uint32_t nseq = 0;     // sequences of the member's batch
    uint32_t waves = 0;    // sequences per workgroup (1, 2 or 4)
    bool grouped = false;  // runs in the set launch (otherwise on its own, after it)
};

struct SetTable {
    std::vector<uint32_t> first;   // [entries + 1]: first block of entry e; first[entries] = the grid
    std::vector<uint32_t> member;  // [entries]: the member entry e belongs to
    uint64_t grid = 0;
    uint32_t entries() const { return (uint32_t)member.size(); }
};

constexpr uint64_t kSetMaxGrid = 0x7FFFFFFFull;

// Builds the table of the grouped members, in member order: ceil(nseq / waves) * nrng blocks each.
// false (and *err, when given) for a grouped member without ranges or sequences or with a workgroup
// width other than 1, 2 or 4, and for a grid past kSetMaxGrid; members that are not grouped are
// skipped whatever they hold.  No grouped member: an empty table, grid 0.
bool build_set_table(const SetMember* members, uint64_t count, SetTable* out, std::string* err = nullptr);

// The table of a launch with one block per sequence of the same members (the set traceback,
// pipe_paths.hip): entry e is the same member as in build_set_table's table and covers nseq blocks,
// whatever the member's ranges and workgroup width.  Refused as there.
bool build_set_row_table(const SetMember* members, uint64_t count, SetTable* out, std::string* err = nullptr);

// The entry of block bx (the last e with first[e] <= bx) and the block's index within it: what the
// kernel's lookup computes, in its chunks of 64.  bx < grid.
void set_table_lookup(const SetTable& t, uint32_t bx, uint32_t* entry, uint32_t* local);

}  // namespace svh
