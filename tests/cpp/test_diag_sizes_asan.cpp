// The diagonal path variant's host-side size helpers (kernels.h) and the per-sequence offset sums
// Batch::load forms from them, under AddressSanitizer + UBSan (host only, no GPU): every record a
// kernel index can reach lies inside the size the helper gives, at the lengths where a word, a
// checkpoint or a block begins, and the sums do not overflow at the longest sequence a batch takes.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "kernels.h"

using namespace svh;

static int failures = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            ++failures;                                                 \
        }                                                               \
    } while (0)

// The highest index of each record that diag.hip writes and the walk reads for a sequence of `len`
// observations on `nrng` ranges (NP = 64 nrng diagonals), from the kernels' own index expressions.
static void check_len(uint64_t len, uint32_t nrng) {
    const uint64_t NP = 64ull * nrng, nst = len - 1;  // steps 1 .. len - 1
    const uint64_t words = diag_mask_words(len, nrng), ck = diag_ckpt_floats(len, nrng), mu = diag_mu_floats(len, nrng),
                   cc = diag_cck_floats(len, nrng), fc = pipe_fck_floats(len);
    // row r = 0 .. len - 2 is bit 31 - r % 32 of word [r / 32][L], L < NP
    if (nst) CHECK(((nst - 1) / 32) * NP + (NP - 1) < words);
    else CHECK(words == 0);
    CHECK(words == (nst + 31) / 32 * NP);
    // checkpoints of observations 0, 32, ... <= len - 1: [t / 32][p], p < NP
    CHECK((nst / kDiagCkptEvery) * NP + (NP - 1) < ck);
    CHECK(ck == (nst / kDiagCkptEvery + 1) * NP);
    // range minima [u][t], t <= len - 1
    CHECK((uint64_t)(nrng - 1) * len + (len - 1) < mu);
    // sink checkpoints [u][t / 32] and F checkpoints [t / 32]
    CHECK((uint64_t)(nrng - 1) * (nst / 32 + 1) + nst / 32 < cc);
    CHECK(nst / 32 < fc);
    CHECK(cc == fc * nrng);
}

int main() {
    const uint64_t lens[] = {1, 2, 3, 31, 32, 33, 34, 63, 64, 65, 66, 96, 97, 128, 129, 3500, 0xFFFFFF00ull};
    const uint32_t rngs[] = {1, 2, 38, 40};
    for (uint64_t len : lens)
        for (uint32_t r : rngs) check_len(len, r);
    CHECK(diag_mask_words(0, 38) == 0 && diag_ckpt_floats(0, 38) == 0 && diag_cck_floats(0, 38) == 0 &&
          diag_mu_floats(0, 38) == 0);
    // Batch::load's running offsets: a batch of the longest sequences at the widest plan
    // (40 ranges) stays far inside 64 bits, and every sequence's block starts where the last ended
    std::vector<uint64_t> off;
    uint64_t pm = 0, pr = 0, pc = 0, dc = 0;
    for (int q = 0; q < 1000; ++q) {
        const uint64_t len = q % 3 == 0 ? 0xFFFFFF00ull : (uint64_t)(q + 1);
        off.push_back(pm);
        const uint64_t w = diag_mask_words(len, 40), m = diag_mu_floats(len, 40), c = diag_ckpt_floats(len, 40),
                       k = diag_cck_floats(len, 40);
        CHECK(pm + w >= pm && pr + m >= pr && pc + c >= pc && dc + k >= dc);
        pm += w;
        pr += m;
        pc += c;
        dc += k;
    }
    CHECK(off.size() == 1000 && off[0] == 0 && off[1] == diag_mask_words(0xFFFFFF00ull, 40));
    CHECK(pm < (1ull << 62) && pr < (1ull << 62) && pc < (1ull << 62));
    CHECK(kDiagPathsLdsMax * 2 <= kMaxLdsBytes);
    std::printf("diag path sizes: %d failures\n", failures);
    if (!failures) std::printf("ok\n");
    return failures ? 1 : 0;
}
