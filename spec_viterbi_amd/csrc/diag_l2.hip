// _spec level 2 on the diagonal plan (gfx950): every chunk of two observations of every row in one
// launch, for models created with SVH_KERNEL_DIAG (Model::diag_l2_on).
//
// The chunk's arithmetic is pipe_kernel.h's step2 (GraphBLAS_spec_impl.cpp:15-36, 66-81), term for
// term and in the same association: with s1, s2 the chunk's symbols, a light position p takes
//     v'_p = min( fl(fl(eb_p(s2) + eb_{p-1}(s1)) + v_{p-2}),
//                 fl(min(fl(eb_p(s2) + ea_{p-1}(s1)), fl(ea_p(s2) + X_FF(s1))) + F) )
// -- ONE score of the previous chunk, position p - 2's.  So the diagonal plan's geometry (diag.hip)
// holds with a lane that advances by two positions per chunk: after chunk c lane l of range r holds
// position p = (64 r + l + 2 c) mod NP (NP = 64 x ranges; positions past the last light row are the
// plan's +inf dummies), and the score it needs is its own previous value x = v_{p-2}.  No exchange,
// no fill, no wait between waves.  Position 0 has eb_0 = +inf, so a lane that wraps past NP - 1
// lands on position 0 or 1 with a chain term of +inf, as the recurrence says.
//
// The lane holding x = v_{p-2} also owns, with q = p - 1, every other term that v_{p-2} or the
// column q enters:
//     F, checked against the speculated F' = fl(fl(X_FF(s2) + X_FF(s1)) + F):
//         (F, m)    fl(fl(X_FF(s2) + A_F(s1)) + x)
//         (q, q-1)  fl(fl(A_F(s2) + eb_q(s1)) + x)
//         (q, F)    fl(fl(A_F(s2) + ea_q(s1)) + F)
//     the margin check of the light rows' speculated (F, m) term (step2's):
//         fl(A_F(s1) + x) >= fl(R + fl(emax2 + R) 2^-20),  R = fl(X_FF(s1) + F)
//     S, the lane's partial c (S = min over lanes, as at level 0: fl(a + .) is monotone):
//         (S, S)    fl(fl(X_SS(s2) + X_SS(s1)) + c)
//         (S, m)    fl(fl(X_SS(s2) + A_S(s1)) + x)
//         (q, q-1)  fl(fl(A_S(s2) + eb_q(s1)) + x)
//         (q, F)    fl(fl(A_S(s2) + ea_q(s1)) + F)
// The diagonals partition the positions, so every m is "p - 2" and every q is "p - 1" of exactly one
// lane per chunk: every term of F's and S's rows is evaluated once.  Models whose S takes a term
// from F (sx) are not planned here (diag_l2_supported): they keep spec2_kernel.
//
// Data: the level-0 table ring ([S][ring + 64 mirror] float2 {ea, eb} in LDS, refilled one group of
// 64 columns per block from PipeModel::dtab) is consumed at two columns per chunk -- a block is 32
// chunks and walks through the ring exactly as a level-0 block of 64 steps does; the lane reads
// {ea, eb} of column p at plane s2 and of column p - 1 at plane s1 (two contiguous ds_read_b64).
// What is uniform per chunk is folded by the builder lane one block ahead into a per-wave stream:
//     {fl(X_FF(s2) + X_FF(s1)), fl(X_SS(s2) + X_SS(s1)), fl(X_FF(s2) + A_F(s1)), fl(X_SS(s2) + A_S(s1))},
//     {A_F(s2), A_S(s2), X_FF(s1), A_F(s1)}, {ring address of (s2, column), of (s1, column - 1)}
// so the F and S halves of a term share an operand register (as one packed add they measured 5 %
// slower than as two single adds).  A check is one v_cmpx, as at level 0: a
// lane that fails switches itself off until the block's end, where the wave notes which lanes are
// left; one barrier per block.  In a full block the reads are issued ahead of their use (the stream
// entry kPS chunks, the ring pairs kPE chunks): the pairs' addresses come from the entry, two LDS
// round trips that the plain form paid per chunk.
//
// A row's nch = (len - 1) / 2 chunks start from the first observation's state in b.v_in (row q) and
// end in b.scores (row q); rows of 0 chunks are copied through.  The last wave of a row to arrive
// combines the ranges' S partials and violation flags into x.viol[q]: flagged rows are re-run by
// spec2_kernel (runtime.cpp), the odd last observation is the tail launch's.
#include "pipe_common.h"

namespace svh {

using namespace dev;
using namespace pipe_dev;

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

// the level-0 ring (diag.hip): five groups of 64 columns and a mirror of the first 64
constexpr uint32_t kDK = 64;          // columns per ring group
constexpr uint32_t kDR = 5 * kDK;     // ring columns
constexpr uint32_t kDRS = kDR + 64;   // slots per symbol plane
constexpr uint32_t kDG = kDR / kDK;   // ring groups
constexpr uint32_t kCP = kDK / 2;     // 16-byte chunks of a plane's group (two columns each)
constexpr uint32_t kLB = kDK / 2;     // chunks per block: a block consumes one group of columns
constexpr uint32_t kDMaxSym = kDiagMaxSym;

#ifndef SVH_DL2_PS
#define SVH_DL2_PS 3
#endif
#ifndef SVH_DL2_PE
#define SVH_DL2_PE 1
#endif
constexpr uint32_t kPS = SVH_DL2_PS;  // chunks a stream entry is read ahead of its use in a full block
constexpr uint32_t kPE = SVH_DL2_PE;  // chunks the ring pairs are read ahead of their use (< kPS)
static_assert(kPE >= 1 && kPE < kPS && kPS < kLB, "prefetch distances");

__device__ __forceinline__ f2 lds_ld2(uint32_t a) {
    return *(const __attribute__((address_space(3))) f2*)(size_t)a;
}
// EXEC &= !(a < b); see diag.hip: the chunks between two exec_collect() calls are straight-line
// code or a wave-uniform loop, fenced off from the all-lanes code around them
__device__ __forceinline__ void check_off(float a, float b) {
    asm volatile("v_cmpx_nlt_f32_e32 vcc, %0, %1" : : "v"(a), "v"(b) : "vcc");
}
// alive &= EXEC; EXEC = all lanes (s_nop 4: five wait states between a write of EXEC and a DPP operation)
__device__ __forceinline__ void exec_collect(uint64_t& alive) {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_and_b64 %0, %0, exec\n\t"
                 "s_mov_b64 exec, -1\n\t"
                 "s_nop 4"
                 : "+s"(alive)
                 :
                 : "scc", "memory");
    __builtin_amdgcn_sched_barrier(0);
}
// One add kept single (an asm statement: the compiler's SLP pass would pack two adjacent adds again)
__device__ __forceinline__ float add1(float a, float b) {
    float r;
    asm("v_add_f32_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

__host__ __device__ constexpr size_t diag_l2_lds(uint32_t W, uint32_t S) {
    // ring [S][kDRS] float2 | symbol template [S][8] | folded constants [W][2][kLB][4] | constants of
    // one symbol [W][2][kLB][4] | ring addresses [W][2][kLB][2] | blocks [W]
    return ((size_t)S * kDRS * 2 + (size_t)S * 8 + (size_t)W * 2 * kLB * 10 + W) * 4;
}

template <int W>
__global__ __launch_bounds__(64 * W) __attribute__((amdgpu_waves_per_eu(2)))
void diag_l2_kernel(PipeModel m, FusedBatch b, PipeScratch x) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint32_t S = m.S, NR = m.nrng, NP = NR * 64;
    float* ring = lds;                                   // [S][kDRS] {ea, eb}
    float* hcr = ring + (size_t)S * kDRS * 2;            // [S][8] stream template of symbol o
    float* ska = hcr + S * 8;                            // [W][2][kLB] {K_FF, K_SS, K_FM, K_SM}
    float* skb = ska + W * 2 * kLB * 4;                  // [W][2][kLB] {A_F(s2), A_S(s2), X_FF(s1), A_F(s1)}
    float* adr = skb + W * 2 * kLB * 4;                  // [W][2][kLB] ring addresses of (s2, 2c), (s1, 2c - 1)
    uint32_t* wnb = reinterpret_cast<uint32_t*>(adr + W * 2 * kLB * 2);  // [W] blocks of wave w

    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t w = (uint32_t)uniform((int)(tid >> 6));
    const uint32_t rg = blockIdx.x % NR, grp = blockIdx.x / NR;
    const uint32_t q = grp * W + w;
    const bool real = q < b.nseq;
    const uint32_t ring_a = lds_addr(ring);

    // stream template: {A_F, A_S, X_FF, X_SS, LDS address of plane o, 0, 0, 0}
    for (uint32_t i = tid; i < S * 8; i += 64 * W) {
        const uint32_t o = i >> 3, k = i & 7u;
        const float* h = m.hc + o * 8;  // A_S A_F X_SS X_FF | X_SF E_F E_S 0
        float v = 0.0f;
        if (k == 0) v = h[1];
        else if (k == 1) v = h[0];
        else if (k == 2) v = h[3];
        else if (k == 3) v = h[2];
        else if (k == 4) v = __builtin_bit_cast(float, ring_a + o * kDRS * 8u);
        hcr[i] = v;
    }

    const uint8_t* __restrict__ sym = b.symbols + (real ? b.sym_off[q] : 0);
    const uint32_t len = real ? (uint32_t)uniform((int)b.end[q]) : 0u;
    const uint32_t nch = len ? (len - 1) / 2 : 0u;  // chunk c = 1 .. nch: observations 2c - 1, 2c
    const uint32_t nb = (nch + kLB - 1) / kLB;
    if (lane == 0) wnb[w] = nb;

    // ---- ring refill (diag.hip): group g = columns u in [kDK g, kDK g + kDK) of this range (table
    // column (64 rg + u) mod NP), every symbol plane; 16-byte chunks over the workgroup
    constexpr uint32_t kT = 64 * W;
    constexpr uint32_t kRep = (kCP * kDMaxSym + kT - 1) / kT;
    const uint32_t nchunk = kCP * S;
    typedef float lvec __attribute__((ext_vector_type(4 * kRep)));  // a vector, not an array: stays in VGPRs
    lvec lreg;
    auto gload = [&](uint32_t g) {
        const uint32_t c0 = (rg * 64 + g * kDK) % NP;
#pragma unroll
        for (uint32_t r = 0; r < kRep; ++r) {
            const uint32_t k = min(tid + r * kT, nchunk - 1);  // unconditional (clamped) loads
            const float4 v = *reinterpret_cast<const float4*>(m.dtab + (size_t)(k / kCP) * NP + c0 + 2 * (k % kCP));
            lreg[4 * r] = v.x;
            lreg[4 * r + 1] = v.y;
            lreg[4 * r + 2] = v.z;
            lreg[4 * r + 3] = v.w;
        }
    };
    auto lwrite = [&](uint32_t g) {
        const uint32_t s0 = (g % kDG) * kDK;
#pragma unroll
        for (uint32_t r = 0; r < kRep; ++r) {
            const uint32_t k = tid + r * kT;
            if (k < nchunk) {
                float* d = ring + ((size_t)(k / kCP) * kDRS + s0 + 2 * (k % kCP)) * 2;
                const float4 v = make_float4(lreg[4 * r], lreg[4 * r + 1], lreg[4 * r + 2], lreg[4 * r + 3]);
                *reinterpret_cast<float4*>(d) = v;
                if (s0 < 64) *reinterpret_cast<float4*>(d + kDR * 2) = v;
            }
        }
    };
    // ---- per-wave stream of block kb (chunks kLB kb + 1 + j): lane j builds entry j from the two
    // symbols it loaded one block earlier
    uint32_t sy1 = 0, sy2 = 0;
    auto symload = [&](uint32_t kb) {
        const uint32_t t2 = 2 * (kb * kLB + 1 + lane), t1 = t2 - 1;
        const uint32_t hi = len ? len - 1 : 0u;
        const bool on = real && lane < kLB;
        sy1 = on ? (uint32_t)sym[t1 < hi ? t1 : hi] : 0u;
        sy2 = on ? (uint32_t)sym[t2 < hi ? t2 : hi] : 0u;
    };
    auto sbuild = [&](uint32_t kb) {
        if (lane < kLB) {
            const uint32_t o1 = sy1 < S ? sy1 : 0u, o2 = sy2 < S ? sy2 : 0u;
            const float4 g1 = *reinterpret_cast<const float4*>(hcr + o1 * 8);  // {A_F, A_S, X_FF, X_SS} of s1
            const float4 g2 = *reinterpret_cast<const float4*>(hcr + o2 * 8);
            const uint32_t p1 = __builtin_bit_cast(uint32_t, hcr[o1 * 8 + 4]), p2 = __builtin_bit_cast(uint32_t, hcr[o2 * 8 + 4]);
            const uint32_t c2 = 2 * (kb * kLB + 1 + lane);  // the lanes' columns: c2 + lane at s2, c2 - 1 + lane at s1
            const uint32_t e = (w * 2 + (kb & 1u)) * kLB + lane;
            *reinterpret_cast<float4*>(ska + e * 4) = make_float4(g2.z + g1.z, g2.w + g1.w, g2.z + g1.x, g2.w + g1.y);
            *reinterpret_cast<float4*>(skb + e * 4) = make_float4(g2.x, g2.y, g1.z, g1.x);
            *reinterpret_cast<float2*>(adr + e * 2) = make_float2(__builtin_bit_cast(float, p2 + (c2 % kDR) * 8u),
                                                                 __builtin_bit_cast(float, p1 + ((c2 - 1) % kDR) * 8u));
        }
    };

    // ---- prologue: groups 0..3 in the ring, group 4 in flight; the stream of block 0
    gload(0);
    lwrite(0);
    gload(1);
    lwrite(1);
    gload(2);
    lwrite(2);
    gload(3);
    lwrite(3);
    gload(4);
    symload(0);
    __syncthreads();  // the symbol template
    sbuild(0);
    symload(1);

    // ---- state before chunk 1: the first observation's vector (the first-step kernel's row q)
    float xv = kInf, F = kInf, c = kInf;
    if (real) {
        const float* vin = b.v_in + (size_t)q * m.n;
        const uint32_t r = m.lrow[rg * 64 + lane];
        xv = r != kNoRow ? vin[r] : kInf;
        F = m.rowF >= 0 ? vin[m.rowF] : kInf;
        c = (rg == 0 && lane == 0 && m.rowS >= 0) ? vin[m.rowS] : kInf;
    }
    __syncthreads();  // ring groups 0..3, wnb
    uint32_t nbmax = 0;
#pragma unroll
    for (int u = 0; u < W; ++u) nbmax = wnb[u] > nbmax ? wnb[u] : nbmax;
    nbmax = (uint32_t)uniform((int)nbmax);

    f2 FC = (f2){F, c};  // the feeder and the lane's sink partial: one packed add advances both
    uint64_t alive = ~0ull;  // lanes whose checks have held so far, collected after every block
    const float emax2 = m.emax2;
    const uint32_t lane8 = lane * 8u;
    // one chunk from its stream entry {ka, kb} and its two ring pairs
    auto compute = [&](const float4& ka, const float4& kb, const f2& E2, const f2& E1) {
        // E2 = {ea_p(s2), eb_p(s2)}, E1 = {ea_q(s1), eb_q(s1)}, q = p - 1
        // the adds one by one (add1: kept from the compiler's own packing)
        const f2 t = (f2){add1(E2.y, E1.y), add1(E2.y, E1.x)};
        const float fx = add1(E2.x, kb.z);
        const float xa = add1(fminf(t.y, fx), FC.x);
        const float xb = add1(t.x, xv);
        const f2 KF = (f2){add1(ka.x, FC.x), add1(ka.y, FC.y)};
        const f2 KM = (f2){add1(ka.z, xv), add1(ka.w, xv)};
        const f2 QB = (f2){add1(add1(kb.x, E1.y), xv), add1(add1(kb.y, E1.y), xv)};
        const f2 QA = (f2){add1(add1(kb.x, E1.x), FC.x), add1(add1(kb.y, E1.x), FC.x)};
        const float nm = fminf(KM.x, fminf(QB.x, QA.x));
        check_off(nm, KF.x);  // the lane fails where nm < F'
        // the margin bound of the light rows' (F, m) term
        const float Rf = kb.z + FC.x;
        const float thr = Rf + (emax2 + Rf) * 0x1p-20f;
        const float Lf = kb.w + xv;
        check_off(Lf, thr);
        const float cn = fminf(fminf(KF.y, KM.y), fminf(QB.y, QA.y));
        xv = fminf(xa, xb);
        FC = (f2){KF.x, cn};
    };
    // a partial block: plain chunks, every read ahead of its use
    auto chunk = [&](uint32_t e) {
        const float4 ka = *reinterpret_cast<const float4*>(ska + e * 4);
        const float4 kb = *reinterpret_cast<const float4*>(skb + e * 4);
        const float2 ad = *reinterpret_cast<const float2*>(adr + e * 2);
        const f2 E2 = lds_ld2(__builtin_bit_cast(uint32_t, ad.x) + lane8);
        const f2 E1 = lds_ld2(__builtin_bit_cast(uint32_t, ad.y) + lane8);
        compute(ka, kb, E2, E1);
    };
    // a full block, software-pipelined: a chunk's stream entry is read kPS chunks and its ring pairs
    // kPE chunks ahead of their use (the pairs' addresses come from the entry: two LDS round trips
    // that the plain form pays per chunk); register slots j % (kPS + 1), j % (kPE + 1).  The
    // scheduler is fenced between a chunk's reads and its arithmetic so that the reads stay ahead.
    auto block = [&](uint32_t e0) {
        constexpr uint32_t NS = kPS + 1, NE = kPE + 1;
        float4 KA[NS], KB[NS];
        float2 AD[NS];
        f2 P2[NE], P1[NE];
        auto sread = [&](uint32_t j) {
            KA[j % NS] = *reinterpret_cast<const float4*>(ska + (e0 + j) * 4);
            KB[j % NS] = *reinterpret_cast<const float4*>(skb + (e0 + j) * 4);
            AD[j % NS] = *reinterpret_cast<const float2*>(adr + (e0 + j) * 2);
        };
        auto eread = [&](uint32_t j) {
            P2[j % NE] = lds_ld2(__builtin_bit_cast(uint32_t, AD[j % NS].x) + lane8);
            P1[j % NE] = lds_ld2(__builtin_bit_cast(uint32_t, AD[j % NS].y) + lane8);
        };
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (uint32_t j = 0; j < kPS; ++j) sread(j);
#pragma unroll
        for (uint32_t j = 0; j < kPE; ++j) eread(j);
#pragma unroll
        for (uint32_t j = 0; j < kLB; ++j) {
            if (j + kPS < kLB) sread(j + kPS);
            if (j + kPE < kLB) eread(j + kPE);
            __builtin_amdgcn_sched_barrier(0);
            compute(KA[j % NS], KB[j % NS], P2[j % NE], P1[j % NE]);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    for (uint32_t k = 0; k < nbmax; ++k) {
        lwrite(k + 4);  // into the slots of group k - 1, which no wave reads any more
        gload(k + 5);
        sbuild(k + 1);  // into the buffer of block k - 1
        symload(k + 2);
        if (k < nb) {
            const uint32_t rem = nch - k * kLB;
            const uint32_t e0 = (w * 2 + (k & 1u)) * kLB;
            // (the collect right behind the chunks -- straight-line code or a loop with a
            // scalar branch -- so that no other branch sees a partial EXEC)
            if (rem >= kLB) {
                block(e0);
                exec_collect(alive);
            } else {
                __builtin_amdgcn_sched_barrier(0);
                for (uint32_t j = 0; j < rem; ++j) chunk(e0 + j);
                exec_collect(alive);
            }
        }
        lds_barrier();
    }

    // ---- scores of the light positions and this wave's partial
    uint32_t last = 0;
    if (real) {
        float* out = b.scores + (size_t)q * m.n;
        const uint32_t r = m.lrow[(rg * 64 + lane + 2 * (nch % NP)) % NP];
        if (r != kNoRow) g_st_score(out + r, xv);  // the re-run and the tail may come from another XCD
        const float cmin = wave_min63(FC.y);
        const bool any_viol = alive != ~0ull;
        if (lane == 63) {
            g_st64(x.part + ((size_t)q * x.G + rg) * 2, ((uint64_t)(any_viol ? 1u : 0u) << 32) | __builtin_bit_cast(uint32_t, cmin));
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const uint32_t d = __hip_atomic_fetch_add(x.done + q, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            last = d == NR - 1 ? 1u : 0u;
        }
        last = readlane_u(last, 63);
    }
    if (last) {  // this wave combines row q: lanes read the ranges' partials
        float C = kInf;
        uint32_t vi = 0;
        for (uint32_t u = lane; u < NR; u += 64) {
            const uint64_t a = g_ld64(x.part + ((size_t)q * x.G + u) * 2);
            C = fminf(C, __builtin_bit_cast(float, (uint32_t)a));
            vi |= (uint32_t)(a >> 32);
        }
        C = wave_min63(C);
        const bool any = __builtin_amdgcn_ballot_w64(vi != 0) != 0;
        if (lane == 63) {
            float* out = b.scores + (size_t)q * m.n;
            if (m.rowF >= 0) g_st_score(out + m.rowF, FC.x);
            if (m.rowS >= 0) g_st_score(out + m.rowS, C);
            x.viol[q] = any ? 1u : 0u;
            __hip_atomic_store(x.done + q, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

template <int W>
const void* diag_l2_ptr() {
    return reinterpret_cast<const void*>(&diag_l2_kernel<W>);
}

}  // namespace

size_t diag_l2_lds_bytes(uint32_t W, uint32_t S) { return diag_l2_lds(W, S); }

bool diag_l2_supported(const PipeModel& m) {
    return m.dtab && m.nrng && !m.wide && !m.sx && m.S > 0 && m.S <= kDMaxSym && (size_t)m.nrng * 64 <= m.P &&
           m.emax2 < kInf && 2 * diag_l2_lds(kDiagMaxWaves, m.S) <= kDiagLdsMax;
}

hipError_t launch_diag_l2(const PipeModel& m, const FusedBatch& b, const PipeScratch& x, hipStream_t stream) {
    if (!diag_l2_supported(m) || !b.v_in || !b.scores || !b.symbols || !b.sym_off || !b.end || !x.part || !x.done ||
        !x.viol || b.nseq > x.rows || x.G < m.nrng)
        return hipErrorInvalidValue;
    if (b.nseq == 0) return hipSuccess;
    const uint32_t W = diag_waves_for(b.nseq);
    const void* fn = W == 4 ? diag_l2_ptr<4>() : W == 2 ? diag_l2_ptr<2>() : diag_l2_ptr<1>();
    const uint64_t grid = ((uint64_t)b.nseq + W - 1) / W * m.nrng;
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const size_t lds = even_placement_lds(grid, m.cus, diag_l2_lds(W, m.S));
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    PipeModel mm = m;
    FusedBatch bb = b;
    PipeScratch xx = x;
    void* args[] = {&mm, &bb, &xx};
    return hipLaunchKernel(fn, dim3((uint32_t)grid), dim3(64 * W), args, lds, stream);
}

}  // namespace svh
