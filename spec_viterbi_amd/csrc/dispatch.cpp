// The one place that decides which kernels run a pass (dispatch.h; DESIGN.md "Dispatch").
#include "dispatch.h"

#include <algorithm>

namespace svh {
namespace {

// The chain / band plan serves every preference but FUSED and GENERIC: for PIPE, PIPE_WIDE and DIAG
// it is the fallback of flagged rows, the path variant and the plan of views without scratch.
bool band_usable(const ModelCaps& c) {
    return c.band_ok && c.kernel_pref != SVH_KERNEL_FUSED && c.kernel_pref != SVH_KERNEL_GENERIC;
}

// Chain, band, fused or generic: what runs where no pipelined or diagonal plan does.  The 4-wave
// chain plan takes scores views of more rows than the chip has CUs -- the rows of the view, not of
// the batch it was cut from.
StepKernel serial_step(const ModelCaps& c, uint32_t rows, bool paths, bool* wide) {
    *wide = false;
    if (band_usable(c) && (!paths || c.band_paths_ok)) {
        *wide = !paths && c.band_wide_ok && rows > c.cu_count;
        return c.band_chain ? StepKernel::Chain : StepKernel::Band;
    }
    return fused_usable(c, paths) ? StepKernel::Fused : StepKernel::Generic;
}

// Scores on a pipelined plan: PIPE / PIPE_WIDE at any width, AUTO by the thresholds.
bool pipe_scores(const ModelCaps& c, uint32_t rows, StepKernel* k) {
    const bool lat = c.pipe_ok && (c.kernel_pref == SVH_KERNEL_PIPE || (c.kernel_pref == SVH_KERNEL_AUTO && rows <= c.pipe_max_nseq));
    const bool wid = c.pipew_ok && (c.kernel_pref == SVH_KERNEL_PIPE_WIDE ||
                                    (c.kernel_pref == SVH_KERNEL_AUTO && !lat && rows >= c.pipew_min_nseq));
    *k = lat ? StepKernel::Pipe : StepKernel::PipeWide;
    return lat || wid;
}

// Decoded paths on a pipelined plan: the latency plan's variant for the batches that give a CU one
// workgroup, the wide plan's beyond; the chain path variant re-runs flagged rows, so it must exist.
bool pipe_paths(const ModelCaps& c, uint32_t rows, StepKernel* k) {
    if (!c.band_paths_ok) return false;
    const bool lat = c.pipe_ok && c.pipe_paths_ok &&
                     (c.kernel_pref == SVH_KERNEL_PIPE || (c.kernel_pref == SVH_KERNEL_AUTO && rows <= c.pipe_max_nseq_paths));
    const bool wid = c.pipew_ok && c.pipew_paths_ok &&
                     (c.kernel_pref == SVH_KERNEL_PIPE_WIDE || (c.kernel_pref == SVH_KERNEL_AUTO && rows > c.pipe_max_nseq_paths));
    *k = lat ? StepKernel::Pipe : StepKernel::PipeWide;
    return lat || wid;
}

// Scores on the diagonal plan: DIAG at any width -- SVH_DIAG=0 only zeroes AUTO's bound, the table
// stays, so a model created with SVH_KERNEL_DIAG still runs it -- and AUTO up to diag_max_nseq.
bool diag_scores(const ModelCaps& c, uint32_t rows) {
    if (!c.pipe_ok || !c.dtab) return false;
    return c.kernel_pref == SVH_KERNEL_DIAG || (c.kernel_pref == SVH_KERNEL_AUTO && rows <= c.diag_max_nseq);
}

// Decoded paths on the diagonal plan: models created with SVH_KERNEL_DIAG only, at any width.
bool diag_paths(const ModelCaps& c) {
    return c.kernel_pref == SVH_KERNEL_DIAG && c.pipe_ok && c.dtab && c.band_paths_ok && c.diag_paths_ok;
}

}  // namespace

PassPlan resolve_pass(const ModelCaps& c, const PassQuery& q) {
    PassPlan p;
    p.step = p.no_diag = serial_step(c, q.rows, q.paths, &p.band_wide);
    // the chain kernel's compact records where its path variant runs, else backpointers (fused and
    // generic); fixed per model: no term here depends on the rows
    p.records = !q.paths ? PathRecords::None : on_band(p.step) ? PathRecords::Chain : PathRecords::Backpointers;
    // A view without scratch never takes a pipelined or diagonal plan: the time-parallel pass launches
    // views of segment rows with none, so it runs chain / band / fused / generic.
    // (A pipelined plan is uploaded only beside a chain / band plan, and every preference that reaches
    // one also reaches that plan: for a model, band_usable holds whenever the rest does.)
    if (q.scratch && band_usable(c)) {
        StepKernel k;
        const bool piped = q.paths ? pipe_paths(c, q.rows, &k) : pipe_scores(c, q.rows, &k);
        if (piped) {
            p.step = p.no_diag = k;
            p.scratch_G = k == StepKernel::PipeWide ? c.pipew_G : c.pipe_G;
            // scores: the latency kernel re-runs flagged rows itself where the model allows; a path
            // pass always hands them to the chain path variant
            p.serial_fallback = q.paths || k == StepKernel::PipeWide || !c.pipe_rerun;
            if (q.paths) p.records = PathRecords::Pipe;
        }
        // The diagonal plan goes first for scores; its path variant is considered only when the
        // pipelined one is not taken.
        if (q.paths ? !piped && diag_paths(c) : diag_scores(c, q.rows)) {
            p.step = StepKernel::Diag;
            // The tail of a level >= 2 pass runs the diagonal kernel even when a pipelined plan
            // answers as well: its scratch then covers both, and svh_batch_plan names the pipelined
            // (or chain) plan and gives only diag_sm for the tail -- no_diag keeps that name.
            p.scratch_G = q.level >= 2 ? std::max(p.scratch_G, c.diag_nrng) : c.diag_nrng;
            p.serial_fallback = q.paths;  // (scores: flagged rows are re-run inside the launch)
            if (q.paths) p.records = PathRecords::Diag;
        }
    }
    if (q.level >= 2 && q.spec_level >= 2) {
        p.chunks = ChunkRoute::Dense;
        if (q.level == 2 && q.spec_level == 2 && q.spec2_on) {
            const bool pipe_l2 = c.pipe_ok && c.pipe_l2_ok && (c.kernel_pref == SVH_KERNEL_AUTO || c.kernel_pref == SVH_KERNEL_PIPE);
            const bool diag_l2 = c.kernel_pref == SVH_KERNEL_DIAG && c.pipe_ok && c.diag_l2_ok;
            p.chunks = pipe_l2 ? ChunkRoute::Spec2Pipe : diag_l2 ? ChunkRoute::Spec2Diag : ChunkRoute::Spec2;
        }
    }
    return p;
}

bool fused_usable(const ModelCaps& c, bool paths) {
    return c.kernel_pref != SVH_KERNEL_GENERIC && (paths ? c.fused_paths : c.fused_scores);
}

ReportedThresholds reported_thresholds(const ModelCaps& c) {
    const int k = c.kernel_pref;
    ReportedThresholds t{0, 0, 0, 0};
    if (c.pipe_ok) {
        t.pipe_max_nseq = k == SVH_KERNEL_PIPE ? 0xFFFFFFFFu : c.pipe_max_nseq;
        t.pipe_max_nseq_paths = k == SVH_KERNEL_PIPE ? 0xFFFFFFFFu : c.pipe_max_nseq_paths;
    }
    if (c.pipew_ok) t.pipew_min_nseq = k == SVH_KERNEL_PIPE_WIDE ? 0u : k == SVH_KERNEL_AUTO ? c.pipew_min_nseq : 0xFFFFFFFFu;
    if (c.dtab) t.diag_max_nseq = k == SVH_KERNEL_DIAG ? 0xFFFFFFFFu : k == SVH_KERNEL_AUTO ? c.diag_max_nseq : 0u;
    return t;
}

int kernel_id(StepKernel k) {
    switch (k) {
        case StepKernel::Fused: return SVH_KERNEL_FUSED;
        case StepKernel::Band: return SVH_KERNEL_BAND;
        case StepKernel::Chain: return SVH_KERNEL_CHAIN;
        case StepKernel::Pipe: return SVH_KERNEL_PIPE;
        case StepKernel::PipeWide: return SVH_KERNEL_PIPE_WIDE;
        case StepKernel::Diag: return SVH_KERNEL_DIAG;
        case StepKernel::Generic: break;
    }
    return SVH_KERNEL_GENERIC;
}

}  // namespace svh
