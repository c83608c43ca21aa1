// The pass resolver (spec_viterbi_amd/csrc/dispatch.cpp) under AddressSanitizer + UBSan: a
// stand-alone host program, no HIP.  Every consistent capability record -- each chain-plan state
// against each pipelined-plan state, a pipelined plan without a chain plan included, which no model
// has -- under every kernel preference, at widths on both sides of every threshold, with and without
// paths, at every level / _spec state and with and without scratch: the invariants the runtime relies
// on, then the named cases of DESIGN.md 5c / 5l / 5n on the capabilities of 2405.chmm.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "dispatch.h"

using namespace svh;

static int failures = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            if (failures < 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static const int kPrefs[] = {SVH_KERNEL_AUTO, SVH_KERNEL_FUSED, SVH_KERNEL_GENERIC, SVH_KERNEL_BAND,
                             SVH_KERNEL_CHAIN, SVH_KERNEL_PIPE, SVH_KERNEL_PIPE_WIDE, SVH_KERNEL_DIAG};

// the numbers of 2405.chmm on a 256-CU device
static ModelCaps numbers() {
    ModelCaps c;
    c.pipe_G = 5;
    c.pipew_G = 19;
    c.diag_nrng = 38;
    c.cu_count = 256;
    c.pipe_max_nseq = 102;
    c.pipe_max_nseq_paths = 51;
    c.pipew_min_nseq = 103;
    c.diag_max_nseq = 52;
    return c;
}

static std::vector<ModelCaps> all_caps() {
    std::vector<ModelCaps> out;
    // chain plan: none, band, chain, chain with path variant, each chain with / without the 4-wave plan
    for (int band = 0; band < 6; ++band)
        for (int fused = 0; fused < 4; ++fused)
            for (int pipe = 0; pipe < 2; ++pipe)
                for (int bits = 0; bits < (pipe ? 8 : 1); ++bits)       // rerun, path variant, level 2
                    for (int wide = 0; wide < (pipe ? 3 : 1); ++wide)   // none, wide plan, with path variant
                        for (int diag = 0; diag < (pipe ? 5 : 1); ++diag) {  // none, table x {paths, level 2}
                            ModelCaps c = numbers();
                            c.band_ok = band > 0;
                            c.band_chain = band > 1;
                            c.band_paths_ok = band == 3 || band == 5;
                            c.band_wide_ok = band >= 4;
                            c.fused_scores = fused & 1;
                            c.fused_paths = (fused & 2) != 0;
                            c.pipe_ok = pipe;
                            c.pipe_rerun = bits & 1;
                            c.pipe_paths_ok = (bits & 2) != 0;
                            c.pipe_l2_ok = (bits & 4) != 0;
                            c.pipew_ok = wide > 0;
                            c.pipew_paths_ok = wide > 1;
                            c.dtab = diag > 0;
                            c.diag_paths_ok = diag > 0 && ((diag - 1) & 1);
                            c.diag_l2_ok = diag > 0 && ((diag - 1) & 2);
                            for (int k : kPrefs) {
                                c.kernel_pref = k;
                                out.push_back(c);
                            }
                        }
    return out;
}

static bool same(const PassPlan& a, const PassPlan& b) {
    return a.step == b.step && a.no_diag == b.no_diag && a.band_wide == b.band_wide && a.serial_fallback == b.serial_fallback &&
           a.scratch_G == b.scratch_G && a.records == b.records && a.chunks == b.chunks;
}

static void check_invariants() {
    const uint32_t rows[] = {0, 1, 2, 4, 51, 52, 53, 102, 103, 104, 255, 256, 257, 4096};
    struct Spec {
        uint32_t level, spec_level;
        bool spec2_on;
    };
    const Spec specs[] = {{0, 0, false}, {1, 1, false}, {0, 2, true}, {2, 0, false}, {2, 2, true},
                          {2, 2, false}, {2, 3, false}, {3, 3, false}, {3, 2, true}};
    uint64_t cells = 0;
    for (const ModelCaps& c : all_caps()) {
        const bool band = c.band_ok && c.kernel_pref != SVH_KERNEL_FUSED && c.kernel_pref != SVH_KERNEL_GENERIC;
        for (int paths = 0; paths < 2; ++paths) {
            PathRecords at_one = PathRecords::None;
            for (uint32_t r : rows)
                for (const Spec& sp : specs)
                    for (int scratch = 0; scratch < 2; ++scratch) {
                        PassQuery q;
                        q.rows = r;
                        q.paths = paths;
                        q.level = sp.level;
                        q.spec_level = sp.spec_level;
                        q.spec2_on = sp.spec2_on;
                        q.scratch = scratch;
                        const PassPlan p = resolve_pass(c, q);
                        ++cells;
                        // total and deterministic
                        CHECK(same(p, resolve_pass(c, q)));
                        CHECK((int)p.step >= 0 && p.step <= StepKernel::Diag && p.no_diag <= StepKernel::Diag);
                        CHECK(p.records <= PathRecords::Diag && p.chunks <= ChunkRoute::Spec2Diag);
                        // no pipelined or diagonal step kernel without scratch, none without its plan,
                        // no pipelined plan without a chain / band plan
                        if (!scratch) CHECK(!on_scratch(p.step) && !on_scratch(p.no_diag));
                        CHECK(on_scratch(p.step) == (p.scratch_G > 0));
                        if (pipelined(p.step) || pipelined(p.no_diag)) CHECK(band);
                        if (p.step == StepKernel::Pipe || p.no_diag == StepKernel::Pipe) CHECK(c.pipe_ok);
                        if (p.step == StepKernel::PipeWide || p.no_diag == StepKernel::PipeWide) CHECK(c.pipew_ok);
                        if (p.step == StepKernel::Diag) CHECK(c.pipe_ok && c.dtab && p.scratch_G >= c.diag_nrng);
                        if (p.step == StepKernel::Pipe) CHECK(p.scratch_G >= c.pipe_G);
                        if (p.step == StepKernel::PipeWide) CHECK(p.scratch_G >= c.pipew_G);
                        if (on_band(p.step)) CHECK(c.band_ok);
                        if (p.step == StepKernel::Fused) CHECK(paths ? c.fused_paths : c.fused_scores);
                        if (c.kernel_pref == SVH_KERNEL_GENERIC) CHECK(p.step == StepKernel::Generic);
                        if (c.kernel_pref == SVH_KERNEL_FUSED) CHECK(p.step == StepKernel::Fused || p.step == StepKernel::Generic);
                        CHECK(p.no_diag != StepKernel::Diag && (p.step == StepKernel::Diag || p.no_diag == p.step));
                        if (p.band_wide) CHECK(c.band_wide_ok && !paths && r > c.cu_count && on_band(p.step));
                        if (p.serial_fallback) CHECK(on_scratch(p.step) && band);
                        if (p.step == StepKernel::PipeWide) CHECK(p.serial_fallback);
                        if (p.step == StepKernel::Pipe && !paths) CHECK(p.serial_fallback == !c.pipe_rerun);
                        // path records consistent with the step kernel
                        CHECK((p.records == PathRecords::None) == !paths);
                        if (paths) {
                            CHECK((p.records == PathRecords::Pipe) == pipelined(p.step));
                            CHECK((p.records == PathRecords::Diag) == (p.step == StepKernel::Diag));
                            CHECK((p.records == PathRecords::Chain) == (p.step == StepKernel::Chain));
                            CHECK((p.records == PathRecords::Backpointers) == !on_band(p.step));
                            CHECK(p.step != StepKernel::Band);
                            if (on_scratch(p.step)) CHECK(p.serial_fallback && c.band_paths_ok);
                            // backpointers or the chain kernel's records: fixed per model
                            if (r == 0 && &sp == &specs[0] && !scratch) at_one = p.records;
                            CHECK((p.records == PathRecords::Backpointers) == (at_one == PathRecords::Backpointers));
                        }
                        // chunk route none iff level <= 1 or spec_level < 2
                        CHECK((p.chunks == ChunkRoute::None) == (sp.level <= 1 || sp.spec_level < 2));
                        if (p.chunks == ChunkRoute::Spec2Pipe) CHECK(c.pipe_ok && c.pipe_l2_ok && sp.spec2_on && sp.level == 2);
                        if (p.chunks == ChunkRoute::Spec2Diag) CHECK(c.kernel_pref == SVH_KERNEL_DIAG && c.diag_l2_ok && sp.spec2_on);
                        if (p.chunks == ChunkRoute::Spec2) CHECK(sp.spec2_on && sp.level == 2 && sp.spec_level == 2);
                    }
        }
    }
    std::printf("%llu cells\n", (unsigned long long)cells);
}

static PassPlan ask(const ModelCaps& c, uint32_t rows, bool paths = false, uint32_t level = 0, bool scratch = true) {
    PassQuery q;
    q.rows = rows;
    q.paths = paths;
    q.level = level;
    q.spec_level = level >= 2 ? level : 0;
    q.spec2_on = level == 2;
    q.scratch = scratch;
    return resolve_pass(c, q);
}

static void check_named_cases() {
    ModelCaps c = numbers();
    c.band_ok = c.band_chain = c.band_paths_ok = c.band_wide_ok = true;
    c.fused_scores = c.fused_paths = true;
    c.pipe_ok = c.pipew_ok = c.dtab = c.pipe_rerun = true;
    c.pipe_paths_ok = c.pipew_paths_ok = c.diag_paths_ok = c.pipe_l2_ok = c.diag_l2_ok = true;
    // AUTO, scores (5l, 5c): the diagonal plan, then the latency plan, then the wide plan
    for (uint32_t r : {1u, 20u, 52u}) {
        const PassPlan p = ask(c, r);
        CHECK(p.step == StepKernel::Diag && p.no_diag == StepKernel::Pipe && p.scratch_G == 38 && !p.serial_fallback);
    }
    for (uint32_t r : {53u, 102u}) {
        const PassPlan p = ask(c, r);
        CHECK(p.step == StepKernel::Pipe && p.scratch_G == 5 && !p.serial_fallback && !p.band_wide);
    }
    for (uint32_t r : {103u, 256u, 257u, 4096u}) {
        const PassPlan p = ask(c, r);
        CHECK(p.step == StepKernel::PipeWide && p.scratch_G == 19 && p.serial_fallback && p.band_wide == (r > 256));
    }
    // ... decoded paths: the latency plan's variant up to pipe_max_nseq_paths, the wide plan's beyond
    CHECK(ask(c, 51, true).step == StepKernel::Pipe && ask(c, 51, true).records == PathRecords::Pipe);
    CHECK(ask(c, 52, true).step == StepKernel::PipeWide && ask(c, 52, true).records == PathRecords::Pipe);
    // ... a view without scratch (the time-parallel pass): the chain plans, by the rows of the view
    CHECK(ask(c, 20, false, 0, false).step == StepKernel::Chain && !ask(c, 20, false, 0, false).band_wide);
    CHECK(ask(c, 300, false, 0, false).step == StepKernel::Chain && ask(c, 300, false, 0, false).band_wide);
    // ... level 2: the chunks on the pipelined plan; the tail on the diagonal kernel under the
    // pipelined plan's name, its scratch covering both
    {
        const PassPlan p = ask(c, 20, false, 2);
        CHECK(p.chunks == ChunkRoute::Spec2Pipe && p.step == StepKernel::Diag && p.no_diag == StepKernel::Pipe && p.scratch_G == 38);
        CHECK(ask(c, 60, false, 2).step == StepKernel::Pipe && ask(c, 60, false, 3).chunks == ChunkRoute::Dense);
    }
    // SVH_KERNEL_DIAG (5l, 5m, 5n): the diagonal plan at any width, its paths, level-2 chunks on it;
    // SVH_DIAG=0 (AUTO's bound 0, the table in place) changes none of it
    for (uint32_t bound : {52u, 0u}) {
        ModelCaps d = c;
        d.kernel_pref = SVH_KERNEL_DIAG;
        d.diag_max_nseq = bound;
        for (uint32_t r : {1u, 52u, 53u, 103u, 300u, 4096u}) {
            CHECK(ask(d, r).step == StepKernel::Diag && ask(d, r).no_diag == StepKernel::Chain && ask(d, r).scratch_G == 38);
            CHECK(ask(d, r, true).step == StepKernel::Diag && ask(d, r, true).records == PathRecords::Diag);
            CHECK(ask(d, r, false, 2).chunks == ChunkRoute::Spec2Diag && ask(d, r, false, 2).step == StepKernel::Diag);
        }
    }
    {
        ModelCaps a = c;  // AUTO with SVH_DIAG=0: no diagonal plan at any width
        a.diag_max_nseq = 0;
        CHECK(ask(a, 1).step == StepKernel::Pipe);
    }
    // SVH_KERNEL_PIPE / PIPE_WIDE at any width; BAND / CHAIN never leave the chain plan
    for (uint32_t r : {1u, 103u, 4096u}) {
        ModelCaps k = c;
        k.kernel_pref = SVH_KERNEL_PIPE;
        CHECK(ask(k, r).step == StepKernel::Pipe && ask(k, r, true).step == StepKernel::Pipe);
        CHECK(ask(k, r, false, 2).chunks == ChunkRoute::Spec2Pipe);
        k.kernel_pref = SVH_KERNEL_PIPE_WIDE;
        CHECK(ask(k, r).step == StepKernel::PipeWide && ask(k, r, true).step == StepKernel::PipeWide);
        CHECK(ask(k, r, false, 2).chunks == ChunkRoute::Spec2);
        k.kernel_pref = SVH_KERNEL_CHAIN;
        CHECK(ask(k, r).step == StepKernel::Chain && ask(k, r, true).records == PathRecords::Chain);
        // SVH_KERNEL_GENERIC: generic everywhere
        k.kernel_pref = SVH_KERNEL_GENERIC;
        for (int scratch = 0; scratch < 2; ++scratch) {
            CHECK(ask(k, r, false, 0, scratch).step == StepKernel::Generic);
            CHECK(ask(k, r, true, 0, scratch).step == StepKernel::Generic);
            CHECK(ask(k, r, true, 0, scratch).records == PathRecords::Backpointers);
            CHECK(ask(k, r, false, 2, scratch).step == StepKernel::Generic && ask(k, r, false, 2, scratch).chunks == ChunkRoute::Spec2);
        }
        k.kernel_pref = SVH_KERNEL_FUSED;
        CHECK(ask(k, r).step == StepKernel::Fused && ask(k, r, true).step == StepKernel::Fused);
    }
    // what svh_model_info reports of the thresholds
    {
        ModelCaps k = c;
        ReportedThresholds t = reported_thresholds(k);
        CHECK(t.pipe_max_nseq == 102 && t.pipe_max_nseq_paths == 51 && t.pipew_min_nseq == 103 && t.diag_max_nseq == 52);
        k.kernel_pref = SVH_KERNEL_DIAG;
        t = reported_thresholds(k);
        CHECK(t.pipe_max_nseq == 102 && t.pipew_min_nseq == 0xFFFFFFFFu && t.diag_max_nseq == 0xFFFFFFFFu);
        k.kernel_pref = SVH_KERNEL_PIPE;
        t = reported_thresholds(k);
        CHECK(t.pipe_max_nseq == 0xFFFFFFFFu && t.pipe_max_nseq_paths == 0xFFFFFFFFu && t.diag_max_nseq == 0);
        k.kernel_pref = SVH_KERNEL_PIPE_WIDE;
        CHECK(reported_thresholds(k).pipew_min_nseq == 0);
        CHECK(reported_thresholds(ModelCaps()).pipe_max_nseq == 0 && reported_thresholds(ModelCaps()).diag_max_nseq == 0);
    }
    CHECK(kernel_id(StepKernel::Generic) == SVH_KERNEL_GENERIC && kernel_id(StepKernel::Diag) == SVH_KERNEL_DIAG &&
          kernel_id(StepKernel::PipeWide) == SVH_KERNEL_PIPE_WIDE && kernel_id(StepKernel::Band) == SVH_KERNEL_BAND);
}

int main() {
    check_invariants();
    check_named_cases();
    std::printf("%d failures\n", failures);
    if (!failures) std::printf("ok\n");
    return failures ? 1 : 0;
}
