// Model sets (runtime.h BatchSet): one batch of sequences against many models, the members on the
// diagonal plan in one launch (diag.hip diag_set_kernel; the block table is set_table.cpp's).
#include <cstring>

#include "runtime.h"

namespace svh {

BatchSet::BatchSet(Model* const* models, uint64_t nmodels, uint64_t nseq_, const uint64_t* offsets, const uint8_t* symbols,
                   uint32_t flags) {
    if (!models || nmodels == 0) throw Error(SVH_E_INVALID, "batch set: no models");
    if (nmodels > 0xFFFFFFFFull) throw Error(SVH_E_UNSUPPORTED, "batch set: too many models");
    if (flags & SVH_BATCH_PATHS) throw Error(SVH_E_UNSUPPORTED, "batch set: decoded paths are not supported on a set (scores only)");
    if (flags & ~(uint32_t)SVH_BATCH_NO_TIMING) throw Error(SVH_E_INVALID, "batch set: unknown flag");
    for (uint64_t i = 0; i < nmodels; ++i) {
        if (!models[i]) throw Error(SVH_E_INVALID, "batch set: null model");
        if (models[i]->device != models[0]->device) throw Error(SVH_E_INVALID, "batch set: every model must be on one device");
    }
    device = models[0]->device;
    cus = models[0]->cu_count;
    timing = (flags & SVH_BATCH_NO_TIMING) == 0;
    // the members record no events of their own: the set's pair spans the whole run
    for (uint64_t i = 0; i < nmodels; ++i)
        members.push_back(std::make_unique<Batch>(models[i], nseq_, offsets, symbols, (uint32_t)SVH_BATCH_NO_TIMING));
    for (auto& b : members) b->set_stream = models[0]->stream;
    nseq = members[0]->nseq;
    std::vector<SetMember> sm(nmodels);
    grouped.assign(nmodels, 0);
    for (uint64_t i = 0; i < nmodels; ++i) {
        const DevicePipePlan* dp = members[i]->set_plan();
        grouped[i] = dp ? 1 : 0;
        sm[i].grouped = dp != nullptr;
        sm[i].nrng = dp ? dp->plan.nrng : 0;
        sm[i].nseq = nseq;
        sm[i].waves = dp ? diag_resolve(diag_caps(dp->view), {nseq}).W : 0;
    }
    std::string err;
    if (!build_set_table(sm.data(), sm.size(), &table, &err)) throw Error(SVH_E_UNSUPPORTED, "batch set: " + err);
    DeviceGuard g(device);
    if (timing) {
        hip_check(hipEventCreate(&ev_start), "hipEventCreate");
        hip_check(hipEventCreate(&ev_stop), "hipEventCreate");
    }
    if (table.entries()) {
        // the descriptor table and first[]: built and uploaded here, once; run() uploads the
        // descriptors again only when a member's scratch moved (a stand-alone run that grew it)
        hipStream_t s = models[0]->stream;
        d_first.upload(table.first.data(), table.first.size() * 4, s);
        d_entries.alloc((size_t)table.entries() * sizeof(DiagSetEntry));
        refresh(s);
        hip_check(diag_set_plan(h_entries.data(), table.first.data(), table.entries(), &launch), "batch set: launch plan");
        hip_check(hipStreamSynchronize(s), "batch set upload");
        for (auto& b : members) b->ran = false;  // (begin_set_run marked them: nothing has run yet)
    }
}

BatchSet::~BatchSet() {
    DeviceGuard g(device);
    if (ev_start) (void)hipEventDestroy(ev_start);
    if (ev_stop) (void)hipEventDestroy(ev_stop);
}

void BatchSet::refresh(hipStream_t s) {
    std::vector<DiagSetEntry> now(table.entries());
    for (uint32_t e = 0; e < table.entries(); ++e) {
        std::memset(&now[e], 0, sizeof(DiagSetEntry));  // (padding too: the comparison below is bytewise)
        members[table.member[e]]->begin_set_run(s, &now[e]);
    }
    if (now.size() == h_entries.size() && std::memcmp(now.data(), h_entries.data(), now.size() * sizeof(DiagSetEntry)) == 0) return;
    h_entries.swap(now);
    hip_check(hipMemcpyAsync(d_entries.ptr, h_entries.data(), h_entries.size() * sizeof(DiagSetEntry), hipMemcpyHostToDevice, s),
              "batch set descriptors H2D");
}

void BatchSet::run(uint32_t level, hipStream_t s) {
    if (level >= 2) throw Error(SVH_E_UNSUPPORTED, "batch set: levels 0 and 1 only (_spec level >= 2 runs per batch)");
    std::lock_guard<std::mutex> lock(mu);
    DeviceGuard g(device);
    if (!s) s = members[0]->model->stream;
    if (timing) hip_check(hipEventRecord(ev_start, s), "hipEventRecord");
    uint64_t n = 0;
    if (table.entries()) {
        refresh(s);
        hip_check(launch_diag_set(h_entries.data(), table.first.data(), table.entries(), d_entries.as<DiagSetEntry>(),
                                  d_first.as<uint32_t>(), cus, s),
                  "diagonal Viterbi kernel (model set)");
        ++n;
    }
    for (size_t i = 0; i < members.size(); ++i)
        if (!grouped[i]) {
            members[i]->run(level, s);
            ++n;
        }
    if (timing) hip_check(hipEventRecord(ev_stop, s), "hipEventRecord");
    last_launches = n;
    ran = true;
}

svh_batchset_info BatchSet::info() {
    std::lock_guard<std::mutex> lock(mu);
    svh_batchset_info i;
    std::memset(&i, 0, sizeof(i));
    i.members = members.size();
    i.grouped = table.entries();
    i.launches = last_launches;
    i.grid = table.grid;
    i.lds_bytes = launch.lds_bytes;
    i.waves = (int32_t)launch.waves;
    return i;
}

float BatchSet::elapsed_ms() {
    std::lock_guard<std::mutex> lock(mu);
    DeviceGuard g(device);
    if (!ran) throw Error(SVH_E_STATE, "no run recorded");
    if (!timing) throw Error(SVH_E_STATE, "batch set created with SVH_BATCH_NO_TIMING: no run events");
    hip_check(hipEventSynchronize(ev_stop), "hipEventSynchronize");
    float ms = 0;
    hip_check(hipEventElapsedTime(&ms, ev_start, ev_stop), "hipEventElapsedTime");
    return ms;
}

}  // namespace svh
