// The diagonal plan's launch resolver (diag_launch.h; DESIGN.md 5l, "Launch geometry").
#include "diag_launch.h"

namespace svh {

uint32_t diag_waves_for(uint64_t nseq) { return nseq >= 4 ? kDiagMaxWaves : nseq >= 2 ? 2u : 1u; }

size_t even_placement_lds(uint64_t grid, uint32_t cus, size_t lds) {
    if (!cus || !grid) return lds;
    const uint64_t per_cu = (grid + cus - 1) / cus;
    if (per_cu * lds > kDiagLdsMax) return lds;
    const size_t cap = (kDiagLdsMax / per_cu) & ~(size_t)511;
    return cap > lds ? cap : lds;
}

bool diag_model_ok(const DiagCaps& c) {
    return c.nrng != 0 && c.SM == 2 && c.S != 0 && c.S <= kDiagMaxSym && (size_t)c.nrng * 64 <= c.P && !c.wide;
}

// The rules in order; each reads only what the rules above it settled.
DiagLaunch diag_resolve(const DiagCaps& c, const DiagQuery& q) {
    DiagLaunch L;
    const auto scores_lds = [&](bool ld, bool quad) { return diag_lds_scores(c.dk, L.W, c.S, c.P, c.sx, L.dm, ld, quad); };
    // 1. sequences per workgroup
    L.W = diag_waves_for(q.nseq);
    const uint64_t groups = (q.nseq + L.W - 1) / L.W;
    // only scores launches of a full build have variants at all
    const bool variants = !q.paths && c.variants;
    // 2. diagonals per lane: two -- ranges of 128 diagonals, half as many waves -- where one per lane
    // would put more than one wave on a SIMD; rows resumed from v_in keep one; dsm forces either
    if (variants && c.dtab2 && c.nrng2) {
        if (c.dsm == 1 || c.dsm == 2) L.dm = c.dsm;
        else if (!q.resumed && c.cus && groups * L.W * c.nrng > 4ull * c.cus) L.dm = 2;
    }
    L.ranges = L.dm == 2 ? c.nrng2 : c.nrng;
    L.grid = groups * L.ranges;
    // 3. the loader wave, if its third stream buffer fits: launches of at most one workgroup per CU (a
    // wave alone on its SIMD has no neighbour to hide the block's other work behind, and the buffer
    // then costs no residency); dld forces either; the floor is a loader-wave launch of full workgroups
    if (variants && q.nseq && scores_lds(true, false) <= kDiagLdsMax) {
        if (q.floor) L.floor = L.loader = L.W == kDiagMaxWaves;
        else if (c.dld) L.loader = c.dld == 2;
        else L.loader = c.cus && L.grid <= c.cus;
    }
    // 4. the quad ring: a two-diagonal loader-wave launch of a model that has the table, if the wider
    // ring fits; dqd = 1 forces it off; the floor reads no ring and keeps the planes
    L.quad = L.loader && !L.floor && L.dm == 2 && c.dtab4 && c.dqd != 1 && c.dk == 64 && scores_lds(true, true) <= kDiagLdsMax;
    // 5. the workgroup and its LDS
    L.threads = 64 * (L.W + (L.loader ? 1 : 0));
    L.lds_bytes = q.paths ? diag_lds_paths(c.dk, L.W, c.S, c.sx) : scores_lds(L.loader, L.quad);
    L.lds_request = even_placement_lds(L.grid, c.cus, L.lds_bytes);
    L.ok = diag_model_ok(c) && (!q.paths || (c.ties_heavy && diag_paths_fit(c.dk, c.variants, c.S, c.sx))) &&
           (L.dm == 1 || (size_t)c.nrng2 * 128 == c.P) && q.floor == L.floor && L.lds_bytes <= kDiagLdsMax &&
           L.grid <= 0x7FFFFFFFull;
    return L;
}

}  // namespace svh
