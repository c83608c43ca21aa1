// Model sets (runtime.h BatchSet): one batch of sequences against many models, the members on the
// diagonal plan in one launch (diag.hip diag_set_kernel; the block table is set_table.cpp's); decoded
// paths of chosen (member, row) pairs in the same manner (diag_set_paths_kernel, pipe_paths.hip
// diag_set_traceback_kernel).
#include <algorithm>
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
    // the sequences themselves, for the decode batches (8-bit symbols: small)
    h_offsets.assign(offsets, offsets + nseq + 1);
    h_symbols.assign(symbols + offsets[0], symbols + offsets[nseq]);
    dec.batch.resize(nmodels);
    dec.rows.assign(nmodels, 0);
    dec.grouped.assign(nmodels, 0);
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
        hip_check(hipEventCreate(&dec_start), "hipEventCreate");
        hip_check(hipEventCreate(&dec_stop), "hipEventCreate");
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
    if (dec_start) (void)hipEventDestroy(dec_start);
    if (dec_stop) (void)hipEventDestroy(dec_stop);
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

// ---- decoded paths of chosen pairs --------------------------------------------------------------

// The decode batches of a new pair list: member i's chosen rows, in list order, as a path batch of its
// own (created on first use, reloaded after: its device buffers only grow), then the two block tables
// of the grouped ones.  Synchronous: the batches' uploads are complete on return.
void BatchSet::decode_build(const uint64_t* member, const uint64_t* row, uint64_t npairs) {
    // a reload reuses the batches' staging and record buffers: their last pass must be over
    if (dec.ran) hip_check(hipStreamSynchronize(dec.stream), "batch set decode: previous pass");
    dec.ran = false;
    dec.fetched = false;
    dec.member.clear();
    dec.row.clear();
    const size_t nm = members.size();
    std::vector<std::vector<uint32_t>> chosen(nm);
    dec.pair_row.resize(npairs);
    for (uint64_t k = 0; k < npairs; ++k) {
        dec.pair_row[k] = (uint32_t)chosen[member[k]].size();
        chosen[member[k]].push_back((uint32_t)row[k]);
    }
    std::vector<SetMember> sm(nm);
    std::vector<uint64_t> offs;
    std::vector<uint8_t> sym;
    uint32_t widest = 0;
    const DevicePipePlan* any = nullptr;
    dec.grouped_pairs = 0;
    for (size_t i = 0; i < nm; ++i) {
        const uint32_t n = (uint32_t)chosen[i].size();
        dec.rows[i] = n;
        dec.grouped[i] = 0;
        if (!n) continue;
        offs.assign(1, 0);
        sym.clear();
        for (uint32_t r : chosen[i]) {
            sym.insert(sym.end(), h_symbols.begin() + (h_offsets[r] - h_offsets[0]), h_symbols.begin() + (h_offsets[r + 1] - h_offsets[0]));
            offs.push_back(sym.size());
        }
        Model* m = members[i]->model;
        if (!dec.batch[i]) {
            dec.batch[i] = std::make_unique<Batch>(m, n, offs.data(), sym.data(), (uint32_t)(SVH_BATCH_PATHS | SVH_BATCH_NO_TIMING));
            dec.batch[i]->set_stream = members[0]->model->stream;
        } else {
            dec.batch[i]->load(n, offs.data(), nullptr, sym.data(), m->stream);
            hip_check(hipStreamSynchronize(m->stream), "batch set decode: upload");
        }
        const DevicePipePlan* dp = dec.batch[i]->set_decode_plan();
        dec.grouped[i] = dp ? 1 : 0;
        sm[i].grouped = dp != nullptr;
        sm[i].nrng = dp ? dp->plan.nrng : 0;
        sm[i].nseq = n;
        if (dp) {
            widest = std::max(widest, n);
            any = dp;
            dec.grouped_pairs += n;
        }
    }
    // one W per launch: what a paths launch of the largest grouped batch would take on its own
    const uint32_t W = any ? diag_resolve(diag_caps(any->view), {widest, false, true}).W : 0;
    for (size_t i = 0; i < nm; ++i) sm[i].waves = sm[i].grouped ? W : 0;
    std::string err;
    if (!build_set_table(sm.data(), sm.size(), &dec.table, &err) || !build_set_row_table(sm.data(), sm.size(), &dec.ttable, &err))
        throw Error(SVH_E_UNSUPPORTED, "batch set decode: " + err);
    dec.h_entries.clear();  // (decode_refresh uploads the descriptors)
    dec.h_tentries.clear();
    dec.launch = DiagSetLaunch{};
    if (dec.table.entries()) {
        hipStream_t s0 = members[0]->model->stream;
        dec.d_first.upload_async(dec.table.first.data(), dec.table.first.size() * 4, s0);
        dec.d_tfirst.upload_async(dec.ttable.first.data(), dec.ttable.first.size() * 4, s0);
        dec.d_entries.reserve((size_t)dec.table.entries() * sizeof(DiagSetEntry));
        dec.d_tentries.reserve((size_t)dec.table.entries() * sizeof(DiagSetTbEntry));
        hip_check(hipStreamSynchronize(s0), "batch set decode: tables");
    }
    dec.member.assign(member, member + npairs);
    dec.row.assign(row, row + npairs);
    ++dec.builds;
}

void BatchSet::decode_refresh(hipStream_t s) {
    const uint32_t ne = dec.table.entries();
    std::vector<DiagSetEntry> now(ne);
    std::vector<DiagSetTbEntry> tnow(ne);
    for (uint32_t e = 0; e < ne; ++e) {
        std::memset(&now[e], 0, sizeof(DiagSetEntry));  // (padding too: the comparisons below are bytewise)
        std::memset(&tnow[e], 0, sizeof(DiagSetTbEntry));
        dec.batch[dec.table.member[e]]->begin_set_decode(s, &now[e], &tnow[e]);
    }
    if (now.size() != dec.h_entries.size() || std::memcmp(now.data(), dec.h_entries.data(), now.size() * sizeof(DiagSetEntry)) != 0) {
        dec.h_entries.swap(now);
        hip_check(hipMemcpyAsync(dec.d_entries.ptr, dec.h_entries.data(), dec.h_entries.size() * sizeof(DiagSetEntry),
                                 hipMemcpyHostToDevice, s),
                  "batch set decode descriptors H2D");
    }
    if (tnow.size() != dec.h_tentries.size() ||
        std::memcmp(tnow.data(), dec.h_tentries.data(), tnow.size() * sizeof(DiagSetTbEntry)) != 0) {
        dec.h_tentries.swap(tnow);
        hip_check(hipMemcpyAsync(dec.d_tentries.ptr, dec.h_tentries.data(), dec.h_tentries.size() * sizeof(DiagSetTbEntry),
                                 hipMemcpyHostToDevice, s),
                  "batch set decode traceback descriptors H2D");
    }
}

void BatchSet::decode(const uint64_t* member, const uint64_t* row, uint64_t npairs, hipStream_t s) {
    if (!member || !row || npairs == 0) throw Error(SVH_E_INVALID, "batch set decode: no pairs");
    if (npairs > 0x7FFFFFFFull) throw Error(SVH_E_UNSUPPORTED, "batch set decode: too many pairs");
    for (uint64_t k = 0; k < npairs; ++k)
        if (member[k] >= members.size() || row[k] >= nseq)
            throw Error(SVH_E_RANGE, "batch set decode: pair " + std::to_string(k) + " (member " + std::to_string(member[k]) + ", row " +
                                         std::to_string(row[k]) + ") out of range");
    std::lock_guard<std::mutex> lock(mu);
    DeviceGuard g(device);
    if (!s) s = members[0]->model->stream;
    const bool same = dec.ran && dec.member.size() == npairs && std::equal(member, member + npairs, dec.member.begin()) &&
                      std::equal(row, row + npairs, dec.row.begin());
    if (!same) decode_build(member, row, npairs);
    if (timing) hip_check(hipEventRecord(dec_start, s), "hipEventRecord");
    uint64_t n = 0;
    const uint32_t ne = dec.table.entries();
    if (ne) {
        // the grouped batches' pass: the forward set launch, each batch's chain path variant over the
        // rows that launch flagged, the set traceback (unflagged rows), each batch's chain traceback
        decode_refresh(s);
        if (dec.launch.grid == 0)
            hip_check(diag_set_plan(dec.h_entries.data(), dec.table.first.data(), ne, &dec.launch, true), "batch set decode: launch plan");
        hip_check(launch_diag_set(dec.h_entries.data(), dec.table.first.data(), ne, dec.d_entries.as<DiagSetEntry>(),
                                  dec.d_first.as<uint32_t>(), cus, s, true),
                  "diagonal Viterbi kernel, path variant (model set)");
        for (uint32_t e = 0; e < ne; ++e) dec.batch[dec.table.member[e]]->set_decode_chain(s);
        hip_check(launch_diag_set_traceback(dec.h_tentries.data(), dec.ttable.first.data(), ne, dec.d_tentries.as<DiagSetTbEntry>(),
                                            dec.d_tfirst.as<uint32_t>(), s),
                  "traceback kernel (model set)");
        for (uint32_t e = 0; e < ne; ++e) dec.batch[dec.table.member[e]]->set_decode_chain_traceback(s);
        n += 2 + 2 * (uint64_t)ne;
    }
    for (size_t i = 0; i < members.size(); ++i)
        if (dec.rows[i] && !dec.grouped[i]) {
            dec.batch[i]->run(0, s);
            ++n;
        }
    if (timing) hip_check(hipEventRecord(dec_stop, s), "hipEventRecord");
    dec.launches = n;
    dec.stream = s;
    dec.ran = true;
    dec.fetched = false;
}

// Every decode batch's results into host memory, once per decode: the scores, best states and paths
// (Batch::read: one synchronisation each, and the batch's fault word) and the rows the chain path
// variant decoded.
void BatchSet::decode_fetch(hipStream_t s) {
    if (!dec.ran) throw Error(SVH_E_STATE, "svh_batchset_decode_read before svh_batchset_decode");
    if (dec.fetched) return;
    const size_t nm = members.size();
    dec.scores.resize(nm);
    dec.best.resize(nm);
    dec.paths.resize(nm);
    dec.fell.resize(nm);
    dec.fallback_pairs = 0;
    for (size_t i = 0; i < nm; ++i) {
        if (!dec.rows[i]) continue;
        Batch& b = *dec.batch[i];
        dec.scores[i].resize((size_t)b.nseq * b.model->host.n);
        dec.best[i].resize(b.nseq);
        dec.paths[i].resize(b.total);
        dec.fell[i].assign(b.nseq, 0);
        b.read(s ? s : dec.stream, dec.scores[i].data(), dec.best[i].data(), dec.paths[i].data());
        dec.fallback_pairs += b.pipe_fallbacks(dec.fell[i].data());
    }
    dec.fetched = true;
}

void BatchSet::decode_read(uint64_t pair, float* scores, int64_t* best, int32_t* path, int32_t* fell_back, hipStream_t s) {
    std::lock_guard<std::mutex> lock(mu);
    DeviceGuard g(device);
    decode_fetch(s);
    if (pair >= dec.member.size()) throw Error(SVH_E_RANGE, "batch set decode: pair index out of range");
    const size_t i = dec.member[pair];
    const uint32_t q = dec.pair_row[pair];
    const Batch& b = *dec.batch[i];
    const uint32_t n = b.model->host.n;
    if (scores) std::memcpy(scores, dec.scores[i].data() + (size_t)q * n, (size_t)n * 4);
    if (best) *best = dec.best[i][q];
    if (path) std::memcpy(path, dec.paths[i].data() + (b.offsets[q] - b.offsets[0]), (size_t)b.lens[q] * 4);
    if (fell_back) *fell_back = dec.fell[i][q] ? 1 : 0;
}

svh_batchset_decode_info BatchSet::decode_info() {
    std::lock_guard<std::mutex> lock(mu);
    DeviceGuard g(device);
    svh_batchset_decode_info i;
    std::memset(&i, 0, sizeof(i));
    i.builds = dec.builds;
    if (!dec.ran) return i;
    decode_fetch(nullptr);
    i.pairs = dec.member.size();
    for (size_t k = 0; k < members.size(); ++k) i.members += dec.rows[k] ? 1 : 0;
    i.grouped = dec.table.entries();
    i.grouped_pairs = dec.grouped_pairs;
    i.launches = dec.launches;
    i.grid = dec.table.grid;
    i.lds_bytes = dec.launch.lds_bytes;
    i.waves = (int32_t)dec.launch.waves;
    i.fallback_pairs = dec.fallback_pairs;
    return i;
}

float BatchSet::decode_elapsed_ms() {
    std::lock_guard<std::mutex> lock(mu);
    DeviceGuard g(device);
    if (!dec.ran) throw Error(SVH_E_STATE, "no decode recorded");
    if (!timing) throw Error(SVH_E_STATE, "batch set created with SVH_BATCH_NO_TIMING: no decode events");
    hip_check(hipEventSynchronize(dec_stop), "hipEventSynchronize");
    float ms = 0;
    hip_check(hipEventElapsedTime(&ms, dec_start, dec_stop), "hipEventElapsedTime");
    return ms;
}

}  // namespace svh
