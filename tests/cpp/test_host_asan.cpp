// Host code of the engine under AddressSanitizer + UBSan (built by `make tests`, run by
// tests/test_readers_asan.py; no GPU is touched): the canonical host model and every plan builder
// of runtime.cpp (fused, band / chain, pipelined latency and wide, on-chip level 2) over every
// committed .chmm and over generated models with malformed and edge-case inputs -- every fused plan
// replayed on the host against the CSR recurrence (replay_fused_plan), with models aimed at each
// fused family, the geometry edges and every workgroup cap -- and the parser
// thread's chunk hand-off of the pipelined file decoder (chunker.cpp) over every .ess and the FASTA
// fixture, with a consumer thread, at several chunkings, including files that fail mid-way.  The
// counterpart of the reference running its whole test suite under valgrind memcheck
// (run_tests.sh:4-7, tests/CMakeLists.txt:4-5).
//   usage: test_host_asan <data dir> <fasta fixture> <scratch dir>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <dirent.h>
#include <fstream>
#include <limits>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "chunker.h"
#include "data_reader.h"
#include "runtime.h"
#include "svh.h"

namespace {

int failures = 0;
int plans_built = 0;

void check(bool ok, const std::string& what) {
    if (!ok) {
        std::fprintf(stderr, "FAIL: %s\n", what.c_str());
        ++failures;
    }
}

std::vector<std::string> list(const std::string& dir, const std::string& ext) {
    std::vector<std::string> out;
    if (DIR* d = opendir(dir.c_str())) {
        while (dirent* e = readdir(d)) {
            const std::string n = e->d_name;
            if (n.size() > ext.size() && n.compare(n.size() - ext.size(), ext.size(), ext) == 0) out.push_back(dir + "/" + n);
        }
        closedir(d);
    }
    return out;
}

struct Coo {  // a model in the C ABI's form (svh_model_create's arrays)
    uint64_t n = 0, S = 0;
    std::vector<uint64_t> scol, src, dst;
    std::vector<float> sval, emis, prob;
};

Coo from_hmm(const HMM& h) {
    Coo c;
    c.n = h.states_num;
    c.S = h.emit_num;
    c.scol.assign(h.start_probabilities_cols.begin(), h.start_probabilities_cols.end());
    c.sval.assign(h.start_probabilities.begin(), h.start_probabilities.end());
    for (const auto& row : h.emissions) c.emis.insert(c.emis.end(), row.begin(), row.end());
    c.src.assign(h.trans_rows.begin(), h.trans_rows.end());
    c.dst.assign(h.trans_cols.begin(), h.trans_cols.end());
    c.prob.assign(h.trans_probs.begin(), h.trans_probs.end());
    return c;
}

svh::HostModel host(const Coo& c) {
    return svh::build_host_model(c.n, c.S, c.scol.size(), c.scol.data(), c.sval.data(), c.emis.data(), c.src.size(),
                                 c.src.data(), c.dst.data(), c.prob.data());
}

int host_error(const Coo& c) {
    try {
        host(c);
    } catch (const svh::Error& e) {
        return e.code;
    }
    return 0;
}

bool same_bits(float a, float b) {  // bit-exact, except that -0.0 == +0.0
    uint32_t x, y;
    std::memcpy(&x, &a, 4);
    std::memcpy(&y, &b, 4);
    return x == y || (a == 0.0f && b == 0.0f);
}

constexpr uint32_t kNone = 0xFFFFFFFFu;
void lex_min(float& v, uint32_t& k, float v2, uint32_t k2) {  // (value, index) minimum, as the kernels'
    if (v2 < v || (v2 == v && k2 < k)) v = v2, k = k2;
}

// One observation evaluated twice, for a few score vectors and every symbol: by the fused kernel's
// schedule from the Plan tables alone (fused_impl.h: light rows from lcol / lval over the LDS index
// space [states | +inf scratch | heavy slots], heavy rows from hval + exceptions, or hmask / hw +
// exceptions in the uniform mode, emissions from emis_pad), and by the CSR recurrence
// min_k fl(fl(E + T) + v[k]).  Values must agree bit for bit; in the general mode (the decoded-path
// plan) the argmin predecessor too, lowest index on ties.
// Returns what differs, or an empty string.
std::string replay_difference(const svh::HostModel& hm, const svh::Plan& p) {
    const uint32_t n = hm.n, S = hm.S, B = p.B, SM = p.SM, R = p.R, est = p.estride;
    const uint32_t scratch = est, hs0 = est + 1;
    const bool general = p.mode == svh::kHeavyGeneral;
    const size_t ndma = (SM + 3) / 4;
    bool sizes = est == SM * B && est >= n && B % 64 == 0 && B <= (uint32_t)svh::kMaxFusedThreads && p.H <= p.HM &&
                 p.HM <= (uint32_t)svh::kMaxHeavy && p.XM <= (uint32_t)svh::kMaxExc && p.vstride >= hs0 + svh::kMaxHeavy &&
                 p.vstride % 4 == 0 && p.lds_bytes == svh::fused_lds_bytes_for((int)SM, B, p.vstride) &&
                 p.lds_bytes <= svh::kMaxLdsBytes && p.lcol.size() == (size_t)SM * R * B && p.lval.size() == p.lcol.size() &&
                 p.emis_pad.size() >= (size_t)(S - 1) * est + ndma * B * 4 && p.start_pad.size() >= est;
    if (general) sizes = sizes && p.hval.size() == (size_t)p.HM * SM * B && p.hvalid.size() == p.hval.size();
    else sizes = sizes && p.hmask.size() == est;
    if (!sizes) return "fused table sizes";
    // what the padding must hold: +inf emissions and start scores past n, every LDS index in range
    bool pads = true;
    for (uint32_t o = 0; o < S; ++o)
        for (uint32_t j = 0; j < est; ++j)
            pads = pads && (j < n ? same_bits(p.emis_pad[(size_t)o * est + j], hm.emis[(size_t)o * n + j])
                                  : std::isinf(p.emis_pad[(size_t)o * est + j]));
    for (uint32_t j = 0; j < est; ++j) pads = pads && (j < n ? same_bits(p.start_pad[j], hm.start[j]) : std::isinf(p.start_pad[j]));
    for (uint32_t c : p.lcol) pads = pads && c < p.vstride && (c < n || c >= scratch) && c < hs0 + std::max(p.H, 1u);
    std::vector<int> hidx(n, -1);
    for (uint32_t h = 0; h < (uint32_t)svh::kMaxHeavy; ++h) {
        pads = pads && p.hrow[h] >= 0 && (uint32_t)p.hrow[h] < n;
        if (h < p.H && pads) hidx[p.hrow[h]] = (int)h;
        for (uint32_t x = 0; x < (uint32_t)svh::kMaxExc; ++x) {
            const uint32_t c = p.xk[h][x];
            pads = pads && c < p.vstride && (c < n || c >= scratch) && (h < p.H || (c == scratch && std::isinf(p.xw[h][x])));
        }
    }
    if (!pads) return "fused padding and index ranges";

    auto source_of = [&](uint32_t c) { return c == scratch ? kNone : c >= hs0 ? (uint32_t)p.hrow[c - hs0] : c; };
    std::mt19937 rng(n * 131u + SM * 7u + p.family);
    std::uniform_real_distribution<float> u(0.0f, 30.0f);
    std::vector<float> v(n), lds(p.vstride);
    for (int trial = 0; trial < 4; ++trial) {
        for (float& x : v)
            x = trial == 0 ? (rng() % 4 ? u(rng) : INFINITY)  // some +inf
                : trial == 1 ? (float)(rng() % 3)            // exact ties
                : trial == 2 ? (rng() % 16 ? INFINITY : u(rng))  // mostly +inf
                             : INFINITY;
        std::fill(lds.begin(), lds.end(), INFINITY);
        std::copy(v.begin(), v.end(), lds.begin());
        for (uint32_t h = 0; h < p.H; ++h) lds[hs0 + h] = v[p.hrow[h]];
        float mu = INFINITY;  // uniform mode: the minimum over the shared source set
        if (!general)
            for (uint32_t k = 0; k < est; ++k) mu = std::fmin(mu, lds[k] + p.hmask[k]);
        for (uint32_t o = 0; o < S; ++o) {
            const float* e = p.emis_pad.data() + (size_t)o * est;
            for (uint32_t j = 0; j < n; ++j) {
                float ref = INFINITY, got = INFINITY;
                uint32_t refk = kNone, gotk = kNone;
                for (uint32_t q = hm.rowptr[j]; q < hm.rowptr[j + 1]; ++q)
                    lex_min(ref, refk, (hm.emis[(size_t)o * n + j] + hm.val[q]) + v[hm.col[q]], hm.col[q]);
                if (hidx[j] < 0) {
                    const uint32_t s = j / B, t = j % B;
                    for (uint32_t r = 0; r < R; ++r) {
                        const size_t idx = ((size_t)s * R + r) * B + t;
                        lex_min(got, gotk, (e[j] + p.lval[idx]) + lds[p.lcol[idx]], source_of(p.lcol[idx]));
                    }
                } else {
                    const uint32_t h = (uint32_t)hidx[j];
                    if (general) {
                        for (uint32_t k = 0; k < est; ++k) {
                            const size_t idx = ((size_t)h * SM + k / B) * B + k % B;
                            lex_min(got, gotk, (e[j] + p.hval[idx]) + lds[k], p.hvalid[idx] ? k : kNone);
                        }
                    } else {
                        got = (e[j] + p.hw[h]) + mu;
                    }
                    for (uint32_t x = 0; x < p.XM; ++x)
                        lex_min(got, gotk, (e[j] + p.xw[h][x]) + lds[p.xk[h][x]], source_of(p.xk[h][x]));
                }
                if (!same_bits(got, ref) || (general && gotk != refk))
                    return "fused schedule differs from the CSR recurrence at row " + std::to_string(j) + ", symbol " +
                           std::to_string(o) + ", family " + std::to_string(p.family) + ": " + std::to_string(got) +
                           " from " + std::to_string(gotk) + " vs " + std::to_string(ref) + " from " + std::to_string(refk);
            }
        }
    }
    // A minimum shows a wrong term only where that term wins, so the terms themselves too: every
    // row's (source, weight) terms read back from the tables are exactly the CSR row, and every
    // padding entry is inert (+inf weight).
    auto wbits = [](float f) {
        uint32_t b;
        std::memcpy(&b, &f, 4);
        return f == 0.0f ? 0u : b;
    };
    std::vector<std::pair<uint32_t, uint32_t>> terms;
    for (uint32_t j = 0; j < n; ++j) {
        terms.clear();
        const std::string row = " of row " + std::to_string(j);
        if (hidx[j] < 0) {
            for (uint32_t r = 0; r < R; ++r) {
                const size_t idx = ((size_t)(j / B) * R + r) * B + j % B;
                if (p.lcol[idx] != scratch) terms.push_back({source_of(p.lcol[idx]), wbits(p.lval[idx])});
                else if (!std::isinf(p.lval[idx])) return "finite weight on a padding term" + row;
            }
        } else {
            const uint32_t h = (uint32_t)hidx[j];
            for (uint32_t k = 0; k < est; ++k) {
                const size_t idx = ((size_t)h * SM + k / B) * B + k % B;
                if (general ? p.hvalid[idx] != 0 : p.hmask[k] == 0.0f) terms.push_back({k, wbits(general ? p.hval[idx] : p.hw[h])});
                else if (!std::isinf(general ? p.hval[idx] : p.hmask[k])) return "finite heavy weight outside the pattern" + row;
            }
            for (uint32_t x = 0; x < p.XM; ++x) {
                if (p.xk[h][x] != scratch) terms.push_back({source_of(p.xk[h][x]), wbits(p.xw[h][x])});
                else if (!std::isinf(p.xw[h][x])) return "finite weight on a padding exception" + row;
            }
        }
        std::sort(terms.begin(), terms.end());
        bool same = terms.size() == hm.rowptr[j + 1] - hm.rowptr[j];
        for (size_t x = 0; same && x < terms.size(); ++x) {
            const uint32_t q = hm.rowptr[j] + (uint32_t)x;
            same = terms[x].first == hm.col[q] && terms[x].second == wbits(hm.val[q]);
        }
        if (!same) return "the tables' terms differ from the CSR's" + row;
    }
    return "";
}

int plans_replayed = 0;
void replay_fused_plan(const svh::HostModel& hm, const svh::Plan& p, const std::string& name) {
    if (!p.fused) return;
    ++plans_replayed;
    const std::string diff = replay_difference(hm, p);
    check(diff.empty(), name + ": " + diff);
}

// the fused planner at one workgroup cap: both variants, replayed
void fused_plans(const svh::HostModel& hm, const std::string& name, int max_threads) {
    for (bool uni : {true, false}) {
        const svh::Plan p = svh::make_plan(hm, max_threads, uni);
        ++plans_built;
        if (p.fused) check(!p.emis_pad.empty() && !p.start_pad.empty(), name + ": fused tables");
        if (p.fused && max_threads > 0) check(p.B <= (uint32_t)max_threads, name + ": workgroup cap");
        if (!uni) check(!p.fused || p.mode == svh::kHeavyGeneral, name + ": path plan is term by term");
        replay_fused_plan(hm, p, name + (uni ? " (scores plan)" : " (path plan)"));
    }
}

// every plan builder over one model, with the invariants a launch relies on
void plans(const svh::HostModel& hm, const std::string& name) {
    const uint32_t n = hm.n;
    check(hm.rowptr.size() == n + 1 && hm.rowptr[n] == hm.col.size() && hm.col.size() == hm.val.size(), name + ": CSR");
    for (uint32_t c : hm.col) check(c < n, name + ": column in range");
    fused_plans(hm, name, 0);
    for (bool chain : {true, false}) {
        const svh::BandPlan b = svh::make_band_plan(hm, 0, chain);
        ++plans_built;
        if (b.ok) check(b.lrow.size() > 0, name + ": band rows");
    }
    for (bool wide : {false, true}) {
        const svh::PipePlan p = svh::make_pipe_plan(hm, 0, 0, wide);
        ++plans_built;
        if (!p.ok) continue;
        check(p.P == p.nblk * 64 * p.SM && p.lrow.size() == p.P && p.start.size() == p.P, name + ": pipe sizes");
        check(p.e0.size() == (size_t)hm.S * p.P && p.hc.size() == (size_t)hm.S * 8, name + ": pipe tables");
        std::vector<uint8_t> seen(n, 0);
        for (uint32_t r : p.lrow)
            if (r != 0xFFFFFFFFu) {
                check(r < n && !seen[r], name + ": pipe position map");
                if (r < n) seen[r] = 1;
            }
        check(p.rowF >= 0 && (uint32_t)p.rowF < n && !seen[p.rowF], name + ": pipe feeder row");
        if (!wide) check(p.emax2 >= 0.0f, name + ": level-2 bound");
    }
    const svh::Spec2Plan s = svh::make_spec2_plan(hm);
    ++plans_built;
    if (s.ok) check(s.la.size() == s.lb.size() && s.lb.size() == s.lv.size() && s.hrow.size() >= 1, name + ": spec2 terms");
}

// MSV-shaped (N = 0, M_1..M_L, C = L + 1) or random models with edge cases
Coo generated(std::mt19937& rng, int kind) {
    std::uniform_real_distribution<float> u(0.0f, 8.0f);
    Coo c;
    const uint64_t L = 1 + rng() % 300;
    c.S = 1 + rng() % (kind == 3 ? 40 : 20);
    if (kind <= 1) {  // chain shape, with chain breaks, +inf terms and duplicates
        c.n = L + 2;
        for (uint64_t j = 1; j <= L; ++j) {
            c.src.push_back(0), c.dst.push_back(j), c.prob.push_back(u(rng));
            if (j < L && rng() % 17) c.src.push_back(j), c.dst.push_back(j + 1), c.prob.push_back(rng() % 9 ? u(rng) : INFINITY);
            c.src.push_back(j), c.dst.push_back(0), c.prob.push_back(1.0f);
            c.src.push_back(j), c.dst.push_back(L + 1), c.prob.push_back(2.0f);
            if (kind == 1 && rng() % 5 == 0) c.src.push_back(j), c.dst.push_back(j + 1 <= L ? j + 1 : 1), c.prob.push_back(u(rng));
        }
        c.src.push_back(0), c.dst.push_back(0), c.prob.push_back(0.5f);
        c.src.push_back(L + 1), c.dst.push_back(L + 1), c.prob.push_back(0.25f);
    } else {  // random out-degree, dense rows, self loops
        c.n = kind == 2 ? 1 + rng() % 3 : L;
        const uint64_t deg = 1 + rng() % 6;
        for (uint64_t a = 0; a < c.n; ++a)
            for (uint64_t k = 0; k < deg; ++k) c.src.push_back(a), c.dst.push_back(rng() % c.n), c.prob.push_back(u(rng));
        for (uint64_t b = 0; b < c.n && c.n > 4; ++b) c.src.push_back(b), c.dst.push_back(0), c.prob.push_back(u(rng));
    }
    c.emis.resize(c.S * c.n);
    for (float& e : c.emis) e = rng() % 13 ? u(rng) : INFINITY;
    c.scol = {0, rng() % c.n, 0};
    c.sval = {u(rng), u(rng), 99.0f};  // a duplicate start column: the first wins
    return c;
}

// A model aimed at one fused family: every light row has R/2 + 1 .. R terms from random sources
// (R itself for exact), H heavy rows take a term from every second or every state, each with its own
// weight, plus terms from their fellow heavy rows and themselves (exception terms, up to XM = H).
Coo aimed(std::mt19937& rng, uint64_t n, uint32_t R, uint32_t H, bool exact) {
    std::uniform_real_distribution<float> u(0.0f, 8.0f);
    Coo c;
    c.n = n;
    c.S = 3;
    std::vector<uint64_t> heavy;
    for (uint32_t h = 0; h < H; ++h) heavy.push_back(h == 0 ? n - 1 : (h * n) / (H + 1));
    auto is_heavy = [&](uint64_t j) { return std::find(heavy.begin(), heavy.end(), j) != heavy.end(); };
    for (uint64_t j = 0; j < n; ++j) {
        if (is_heavy(j)) continue;
        const uint32_t deg = std::min<uint64_t>(n, exact ? R : R / 2 + 1 + rng() % (R - R / 2));
        const uint64_t first = rng() % n, stride = 1 + rng() % 7;  // distinct sources: gcd(stride, n) may exceed 1
        std::vector<uint64_t> used;
        for (uint64_t k = first; used.size() < deg; k = (k + stride) % n) {
            while (std::find(used.begin(), used.end(), k) != used.end()) k = (k + 1) % n;
            used.push_back(k);
            c.src.push_back(k), c.dst.push_back(j), c.prob.push_back(rng() % 11 ? u(rng) : INFINITY);
        }
    }
    for (size_t x = 0; x < heavy.size(); ++x) {
        for (uint64_t k = x % 2; k < n; k += 1 + x % 2)
            if (!is_heavy(k)) c.src.push_back(k), c.dst.push_back(heavy[x]), c.prob.push_back(u(rng));
        for (size_t y = 0; y < heavy.size(); ++y)
            if (y != x || x % 2 == 0) c.src.push_back(heavy[y]), c.dst.push_back(heavy[x]), c.prob.push_back(u(rng));
    }
    c.emis.resize(c.S * c.n);
    for (float& e : c.emis) e = rng() % 13 ? u(rng) : INFINITY;
    c.scol = {0, heavy.empty() ? 1 % n : heavy[0]};
    c.sval = {u(rng), u(rng)};
    return c;
}

// the parser thread's hand-off with a consumer thread: the sequences, in file order
std::vector<std::vector<uint8_t>> chunked(const std::string& path, int fmt, uint64_t ms, uint64_t mx, size_t cap,
                                          int* err) {
    svh::SeqReader reader(path, fmt);
    svh::ChunkQueue queue(cap);
    std::thread producer([&] { svh::produce_chunks(reader, queue, ms, mx); });
    std::vector<std::vector<uint8_t>> out;
    uint64_t next_first = 0;
    *err = 0;
    try {
        svh::Chunk c;
        while (queue.pop(c)) {
            check(c.first == next_first, path + ": chunk order");
            check(!c.offsets.empty() && c.offsets.back() == c.symbols.size(), path + ": chunk offsets");
            for (size_t q = 0; q + 1 < c.offsets.size(); ++q)
                out.emplace_back(c.symbols.begin() + c.offsets[q], c.symbols.begin() + c.offsets[q + 1]);
            next_first += c.offsets.size() - 1;
        }
    } catch (const svh::Error& e) {
        *err = e.code;
    }
    queue.stop();
    producer.join();
    return out;
}

void write(const std::string& path, const std::string& text) { std::ofstream(path) << text; }

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s <data dir> <fasta fixture> <scratch dir>\n", argv[0]);
        return 2;
    }
    const std::string data = argv[1], fasta = argv[2], tmp = argv[3];

    // every committed model: host CSR and every plan
    const auto models = list(data + "/chmm_files", ".chmm");
    check(models.size() >= 20, "expected the reference's .chmm files");
    for (const auto& f : models) {
        const HMM h = read_HMM(f);
        plans(host(from_hmm(h)), f);
    }
    // generated models (chain shapes with breaks / +inf / duplicates, tiny and random ones)
    std::mt19937 rng(20261018);
    for (int i = 0; i < 240; ++i) {
        const Coo c = generated(rng, i % 4);
        plans(host(c), "generated #" + std::to_string(i));
    }
    // models aimed at each fused family and at the geometry edges (n around SM * B, the largest
    // fused model and the first one past it), at every workgroup cap
    {
        std::mt19937 r3(20261019);
        int i = 0;
        for (uint64_t n : {63, 64, 65, 511, 512, 513, 1024, 1025, 1600, 4096, 6143, 6144, 6145})
            for (uint32_t R : {2u, 4u, 8u, 16u}) {
                const uint32_t H = R == 2 ? (i % 2) * 2 : (uint32_t[]){0, 1, 4, 2}[i % 4];
                const bool exact = i % 3 == 0;
                ++i;
                const svh::HostModel hm = host(aimed(r3, n, R, H, exact));
                const std::string name = "aimed n=" + std::to_string(n) + " R=" + std::to_string(R) + " H=" + std::to_string(H);
                const svh::Plan p = svh::make_plan(hm, 0, false);
                const int fam = R == 2 ? svh::kFamR2 : R == 4 ? svh::kFamR4 : R == 8 ? svh::kFamR8 : svh::kFamR16;
                check(p.fused == (n <= 6144), name + ": fused up to 6144 states");
                if (p.fused) check(p.family == fam && p.H == H && p.R == R, name + ": family and heavy rows");
                if (n == 6143 || n == 6144) check(p.SM == 12 && p.B == 512 && p.lds_bytes == 151952, name + ": largest geometry");
                for (int threads : {64, 128, 256, 0}) fused_plans(hm, name + " threads=" + std::to_string(threads), threads);
            }
    }
    // the replay itself: one wrong entry in a copy of any table of a plan must show
    {
        std::mt19937 r4(5);
        const svh::HostModel hm = host(aimed(r4, 700, 4, 2, false));
        const svh::Plan gen = svh::make_plan(hm, 0, false);
        check(gen.fused && gen.H == 2 && gen.SM == 2 && replay_difference(hm, gen).empty(), "replay: the intact plan");
        const uint32_t hr = (uint32_t)gen.hrow[1], est = gen.estride;
        auto spoiled = [&](const char* what, auto&& edit) {
            svh::Plan q = gen;
            edit(q);
            check(!replay_difference(hm, q).empty(), std::string("replay misses a wrong ") + what);
        };
        const size_t lterm = std::find_if(gen.lval.begin(), gen.lval.end(), [](float w) { return !std::isinf(w); }) - gen.lval.begin();
        const size_t hterm = std::find(gen.hvalid.begin(), gen.hvalid.end(), 1) - gen.hvalid.begin();
        spoiled("lval", [&](svh::Plan& q) { q.lval[lterm] += 0.5f; });
        spoiled("lcol", [&](svh::Plan& q) { q.lcol[lterm] = q.lcol[lterm] == 3 ? 4 : 3; });
        spoiled("lcol padding", [&](svh::Plan& q) { *std::find(q.lcol.begin(), q.lcol.end(), est) = est + 5; });
        spoiled("hval", [&](svh::Plan& q) { q.hval[hterm] += 0.5f; });
        spoiled("hvalid", [&](svh::Plan& q) { q.hvalid[hterm] = 0; });
        spoiled("xk", [&](svh::Plan& q) { q.xk[0][0] = est; });
        spoiled("xw", [&](svh::Plan& q) { q.xw[1][0] += 0.25f; });
        spoiled("hrow", [&](svh::Plan& q) { q.hrow[1] = (int)(hr ? hr - 1 : 1); });
        spoiled("emis_pad", [&](svh::Plan& q) { q.emis_pad[est + 7] += 1.0f; });
        spoiled("emis_pad padding", [&](svh::Plan& q) { q.emis_pad[est - 1] = 0.0f; });
        spoiled("estride", [&](svh::Plan& q) { q.estride += 64; });
        const svh::HostModel chain = host(generated(r4, 0));
        const svh::Plan uni = svh::make_plan(chain, 0, true);
        check(uni.fused && uni.mode == svh::kHeavyUniform && replay_difference(chain, uni).empty(), "replay: the intact uniform plan");
        for (int what = 0; what < 3; ++what) {
            svh::Plan q = uni;
            if (what == 0) q.hw[0] += 0.5f;
            if (what == 1) q.hmask[1] = INFINITY;  // M_1 leaves the shared source set
            if (what == 2) q.xw[0][0] += 0.5f;
            check(!replay_difference(chain, q).empty(), "replay misses a wrong uniform table " + std::to_string(what));
        }
    }
    // malformed inputs: the documented errors, never a crash or an out-of-bounds access
    {
        std::mt19937 r2(7);
        const Coo base = generated(r2, 0);
        Coo c = base;
        c.prob[0] = std::numeric_limits<float>::quiet_NaN();
        check(host_error(c) == SVH_E_INVALID, "NaN transition score");
        c = base;
        c.emis[3] = -INFINITY;
        check(host_error(c) == SVH_E_INVALID, "-inf emission score");
        c = base;
        c.dst[1] = c.n;
        check(host_error(c) == SVH_E_RANGE, "transition index out of range");
        c = base;
        c.scol[1] = c.n + 5;
        check(host_error(c) == SVH_E_RANGE, "start index out of range");
        c = base;
        c.S = 257;
        c.emis.resize(c.S * c.n, 1.0f);
        check(host_error(c) == SVH_E_UNSUPPORTED, "more than 256 symbols");
        c = base;
        c.n = 0;
        check(host_error(c) == SVH_E_INVALID, "no states");
        c = base;
        c.src.clear(), c.dst.clear(), c.prob.clear();
        plans(host(c), "no transitions");
        c = base;
        c.scol.clear(), c.sval.clear();
        plans(host(c), "no start states");
    }

    // the file decoder's chunk hand-off over every .ess and the FASTA fixture
    std::vector<std::pair<std::string, int>> files;
    for (const auto& f : list(data + "/ess_files", ".ess")) files.push_back({f, SVH_FORMAT_ESS});
    files.push_back({fasta, SVH_FORMAT_FASTA});
    for (const auto& [path, fmt] : files) {
        int err = 0;
        const auto whole = chunked(path, fmt, 1u << 30, 1ull << 40, 2, &err);
        check(err == 0 && !whole.empty(), path + ": whole file");
        for (auto [ms, mx, cap] : {std::tuple<uint64_t, uint64_t, size_t>{1, 1, 1}, {3, 100, 2}, {7, 5000, 1}, {64, 1u << 20, 4}}) {
            const auto got = chunked(path, fmt, ms, mx, cap, &err);
            check(err == 0 && got == whole, path + ": chunked " + std::to_string(ms) + "/" + std::to_string(mx));
        }
    }
    // a file that fails mid-way: the chunks before the error arrive, then the error
    write(tmp + "/bad.fasta", ">a\nACDE\n>b\nAC*D\n");
    {
        int err = 0;
        const auto got = chunked(tmp + "/bad.fasta", SVH_FORMAT_FASTA, 1, 1u << 20, 2, &err);
        check(err == SVH_E_RANGE && got.size() == 1, "FASTA error after one sequence");
    }
    write(tmp + "/bad.ess", "3\n0 4\n1 2\n");
    {
        int err = 0;
        chunked(tmp + "/bad.ess", SVH_FORMAT_ESS, 1, 1u << 20, 1, &err);
        check(err != 0, "truncated .ess");
    }
    // the consumer stopping early (a callback that returns non-zero): the producer unblocks
    for (const auto& [path, fmt] : files) {
        svh::SeqReader reader(path, fmt);
        svh::ChunkQueue queue(1);
        std::thread producer([&] { svh::produce_chunks(reader, queue, 1, 1u << 20); });
        svh::Chunk c;
        check(queue.pop(c), path + ": first chunk");
        queue.stop();
        producer.join();
    }
    check(plans_replayed >= 2 * (int)models.size(), "every reference model has a fused plan to replay");
    std::printf("host asan: %zu models, %d plans built, %d fused plans replayed, %zu files chunked, %d failures\n",
                models.size(), plans_built, plans_replayed, files.size(), failures);
    return failures ? 1 : 0;
}
