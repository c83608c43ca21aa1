// The launch of the diagonal plan ("Launch geometry"): plain host code, no HIP, as
// dispatch.h.  resolve_pass says that a pass runs the diagonal plan; diag_resolve says which variant
// of diag.hip's kernel that launch is, its grid, its workgroup and its LDS.  launch_diag launches what
// it returns, Model::info reports it, Batch::step_floor_ms asks it for the floor: nothing else decides
// any of it.  The LDS layouts below are the kernels' own (diag_body.h computes its offsets with them).
#pragma once

#include <cstddef>
#include <cstdint>

namespace svh {

constexpr size_t kDiagLdsMax = 160 * 1024;  // a CU's LDS
constexpr uint32_t kDiagMaxWaves = 4;       // sequences (step waves) of the widest workgroup
constexpr uint32_t kDiagMaxSym = 32;        // the ring's symbol planes
constexpr uint32_t kDiagFoldSteps = 8;      // PATHS: steps between two folds of a wave's scores (diag.hip kFS)

// Main LDS of diag_viterbi_kernel for blocks of dk steps:
// ring [S][5 dk + 64] float2 (dm = 2: [S][2][5 dk + 128] floats; quad: [S][5 dk + 64] float4) | symbol
// template [S][8] | constants [W][2][dk][4] | ring addresses [W][2][dk] | X_SF [W][2][dk] (sx only) |
// blocks [W] | rerun rows [W]  (ld, the loader-wave variant: three stream buffers instead of two)
constexpr size_t diag_lds_main(uint32_t dk, uint32_t W, uint32_t S, bool sx, uint32_t dm, bool ld, bool quad) {
    const size_t slots = quad ? (5 * dk + 64) * 2 : dm == 2 ? 5 * dk + 128 : 5 * dk + 64;  // pairs of floats per symbol
    return ((size_t)S * slots * 2 + (size_t)S * 8 + (size_t)W * (ld ? 3 : 2) * dk * (4 + 1 + (sx ? 1 : 0)) + 2 * W) * 4;
}
// Decoded paths: the fold ring [W][kDiagFoldSteps][64] floats behind the plain layout, 16-byte aligned.
constexpr size_t diag_lds_paths(uint32_t dk, uint32_t W, uint32_t S, bool sx) {
    return ((diag_lds_main(dk, W, S, sx, 1, false, false) + 15) & ~(size_t)15) + (size_t)W * kDiagFoldSteps * 64 * 4;
}
// A scores launch's footprint: pipe_rerun_row (v[2][P], red[2][W]) runs in the same LDS.
constexpr size_t diag_lds_scores(uint32_t dk, uint32_t W, uint32_t S, uint32_t P, bool sx, uint32_t dm, bool ld, bool quad) {
    const size_t rerun = (2 * (size_t)P + 2 * W) * 4, mainb = diag_lds_main(dk, W, S, sx, dm, ld, quad);
    return mainb > rerun ? mainb : rerun;
}
// Does the widest plain launch of a layout (dm diagonals per lane) fit: what uploads dtab / dtab2.
// (With the X_SF stream, whatever the model: the larger of the two kernels'.)
constexpr bool diag_widest_fits(uint32_t dk, uint32_t S, uint32_t P, uint32_t dm) {
    return diag_lds_scores(dk, kDiagMaxWaves, S, P, true, dm, false, false) <= kDiagLdsMax;
}
// Whether any quad launch of a model can fit (the narrowest workgroup's): what uploads dtab4.
constexpr bool diag_quad_fits(uint32_t dk, bool variants, uint32_t S, uint32_t P, bool sx) {
    return variants && dk == 64 && diag_lds_scores(dk, 1, S, P, sx, 2, true, true) <= kDiagLdsMax;
}
// The path variant keeps two workgroups on a CU at every width (the headline's 494 workgroups need
// them on 256 CUs): a model whose LDS does not allow that is not planned on it; nor is one whose S
// takes a term from F (sx: no such instantiation, diag.hip diag_kernel).
constexpr size_t kDiagPathsLdsMax = 80 * 1024;
constexpr bool diag_paths_fit(uint32_t dk, bool variants, uint32_t S, bool sx) {
    return !sx && variants && dk == 64 && S > 0 && S <= kDiagMaxSym && diag_lds_paths(dk, kDiagMaxWaves, S, sx) <= kDiagPathsLdsMax;
}

// Even placement: a launch that fits the chip gets its LDS request raised so that no CU can take
// more than ceil(grid / CUs) of its workgroups (the dispatcher would otherwise stack up to four on
// some CUs and leave others empty; the kernel ends with its most loaded CU).  cus = 0: off.
size_t even_placement_lds(uint64_t grid, uint32_t cus, size_t lds);

// What the resolver needs of a model (PipeModel) and of the build (diag.hip fills it: diag_caps).
struct DiagCaps {
    uint32_t S = 0, P = 0, nrng = 0, nrng2 = 0;
    bool sx = false;
    uint32_t cus = 0;
    bool dtab2 = false, dtab4 = false;  // the plane table / the quad table is uploaded
    bool ties_heavy = false;
    uint32_t SM = 0;
    bool wide = false;
    uint32_t dsm = 0, dld = 0, dqd = 0;  // SVH_DIAG_SM / _LOADER / _QUAD at model creation (kernels.h)
    uint32_t dk = 64;                    // the build's block length (diag.hip kDK)
    bool variants = true;                // the build has more than the plain kernel (no diagnostic build)
};
struct DiagQuery {
    uint64_t nseq = 0;
    bool resumed = false;  // rows resume from v_in (the _spec tail, time-parallel segments)
    bool paths = false;    // decoded paths
    bool floor = false;    // the plan's floor (diag.hip FL): svh_batch_step_floor_ms
};
struct DiagLaunch {
    bool ok = false;       // a launch the kernels take (else the other fields say what was tried)
    uint32_t W = 1;        // sequences per workgroup
    uint32_t dm = 1;       // diagonals per lane
    bool loader = false, quad = false, floor = false;
    uint32_t ranges = 0;   // workgroups per W sequences: nrng, with two diagonals per lane nrng2
    uint64_t grid = 0;
    uint32_t threads = 0;
    size_t lds_bytes = 0;    // the variant's own footprint
    size_t lds_request = 0;  // ... after even placement: what the launch asks for
};

uint32_t diag_waves_for(uint64_t nseq);  // the W rule (diag_l2.hip's launch shares it)
// A model the diagonal kernels take at all (any variant, any width).
bool diag_model_ok(const DiagCaps& c);
DiagLaunch diag_resolve(const DiagCaps& c, const DiagQuery& q);

}  // namespace svh
