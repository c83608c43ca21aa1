// Which kernels run a pass (DESIGN.md "Dispatch"): plain host code, no HIP.  Model::Model fills a
// ModelCaps once; every consumer -- Batch::load / run, Model::launch_steps, Model::info, the
// time-parallel pass, the step floor, the model sets -- asks resolve_pass and decides nothing itself.
// The resolver chooses a plan, not a grid: the diagonal plan's launch is diag_resolve's (diag_launch.h);
// waves, slots and LDS sizes of the pipelined and wide plans stay with their kernels (pipew_waves_for, ...).
#pragma once

#include <cstdint>

#include "svh.h"

namespace svh {

// What a model can run.  Fixed at model creation: the environment overrides are already applied and
// every *_supported() answer of the kernel translation units is taken once.
struct ModelCaps {
    int kernel_pref = SVH_KERNEL_AUTO;  // svh_model_opts.kernel
    // the plans the model has
    bool band_ok = false;        // chain / band plan (Model::band)
    bool band_chain = false;     // ... it runs the chain kernel (else band.hip)
    bool band_paths_ok = false;  // ... its decoded-path variant exists (BandPlan::paths_ok)
    bool band_wide_ok = false;   // the 4-wave streamed-E chain plan (Model::band_wide)
    bool fused_scores = false;   // a fused family fits (Model::fast_plan)
    bool fused_paths = false;    // ... term by term, for backpointers (Model::paths_plan)
    bool pipe_ok = false;        // pipelined latency plan (Model::pipe)
    bool pipew_ok = false;       // wide pipelined plan (Model::pipe_wide)
    bool dtab = false;           // the latency plan carries the diagonal table
    uint32_t pipe_G = 0;         // workgroups per sequence of the latency plan
    uint32_t pipew_G = 0;        // blocks per sequence of the wide plan
    uint32_t diag_nrng = 0;      // ranges per sequence of the diagonal plan
    bool pipe_rerun = false;     // the latency kernel re-runs flagged rows itself (PipeModel::rerun)
    uint32_t cu_count = 0;
    // AUTO's thresholds in rows
    uint32_t pipe_max_nseq = 0;        // latency plan, scores: at most
    uint32_t pipe_max_nseq_paths = 0;  // latency plan, decoded paths: at most (the wide plan beyond)
    uint32_t pipew_min_nseq = 0;       // wide plan, scores: at least
    uint32_t diag_max_nseq = 0;        // diagonal plan, scores: at most
    // variants
    bool pipe_paths_ok = false;   // the latency plan's path variant is built and its walk fits the traceback
    bool pipew_paths_ok = false;  // the wide plan's (and SVH_PIPEW_PATHS is not 0)
    bool diag_paths_ok = false;   // the diagonal plan's: F wins every tie and feeds no term to S, at most 32
                                  // symbols, the walk fits the traceback, two workgroups per CU
    bool pipe_l2_ok = false;      // pipe_l2.hip takes the latency plan (every score >= 0, ...)
    bool diag_l2_ok = false;      // diag_l2.hip takes the diagonal table
};

struct PassQuery {
    uint32_t rows = 0;        // rows of the view the step kernel is launched over
    bool paths = false;       // decoded paths (SVH_BATCH_PATHS)
    uint32_t level = 0;       // the level of the run
    uint32_t spec_level = 0;  // Model::spec_level and spec2_on: they change in spec_build, so they are
    bool spec2_on = false;    // no caps
    bool scratch = false;     // the view brings pipelined scratch (PipeScratch)
};

enum class StepKernel { Generic, Fused, Band, Chain, Pipe, PipeWide, Diag };
enum class PathRecords { None, Backpointers, Chain, Pipe, Diag };
enum class ChunkRoute { None, Dense, Spec2, Spec2Pipe, Spec2Diag };

struct PassPlan {
    StepKernel step = StepKernel::Generic;  // the per-observation kernel of the pass (at level >= 2: of its tail)
    // step with the diagonal plan left out: what svh_batch_plan names at level >= 2, and the plan
    // the step floor measures where the diagonal plan's floor launch does not apply
    StepKernel no_diag = StepKernel::Generic;
    bool band_wide = false;  // the chain plan of the pass -- its step kernel, or the serial fallback of a
                             // pipelined one -- is Model::band_wide
    bool serial_fallback = false;  // a second launch re-runs flagged rows on the chain / band kernel
    uint32_t scratch_G = 0;        // PipeScratch groups per row the pass needs (0: no scratch)
    PathRecords records = PathRecords::None;
    ChunkRoute chunks = ChunkRoute::None;  // level >= 2: what evaluates the chunks before the tail
};

inline bool pipelined(StepKernel k) { return k == StepKernel::Pipe || k == StepKernel::PipeWide; }
inline bool on_scratch(StepKernel k) { return pipelined(k) || k == StepKernel::Diag; }
inline bool on_band(StepKernel k) { return k != StepKernel::Generic && k != StepKernel::Fused; }  // Model::band / band_wide is in play

PassPlan resolve_pass(const ModelCaps& caps, const PassQuery& q);

// A fused plan the preference lets run (svh_model_info reports its family under a chain plan too).
bool fused_usable(const ModelCaps& caps, bool paths);

// SVH_KERNEL_* of a step kernel, as svh_model_info reports it.
int kernel_id(StepKernel k);

// AUTO's thresholds as svh_model_info reports them: 0 for a plan the model does not have; where the
// preference forces a plan, its bound at "any width" (0xFFFFFFFF; pipew_min_nseq: 0); pipew_min_nseq
// and diag_max_nseq at "no width" under every other preference but AUTO.
struct ReportedThresholds {
    uint32_t pipe_max_nseq, pipe_max_nseq_paths, pipew_min_nseq, diag_max_nseq;
};
ReportedThresholds reported_thresholds(const ModelCaps& caps);

}  // namespace svh
