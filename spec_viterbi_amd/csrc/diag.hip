// Diagonal plan of the chain Viterbi step (gfx950): the scores path of MSV-shaped models
// (kernels.h, PipeModel) for batches up to a few hundred sequences.
//
// Reference hot loop: Viterbi_impl/GraphBLAS_impl.cpp:59-73 (same association, bit-identical):
//     v'[j] = min_k fl( fl(E[o][j] + T^T[j][k]) + v[k] )
// For the light rows of the chain shape, with F's light term speculated away as in pipe_kernel.h
// (F'(t) = fl(X_FF(o_t) + F'(t-1)), checked exactly at every observation),
//     v_p(t) = min( fl(eb_p(o_t) + v_{p-1}(t-1)), fl(ea_p(o_t) + F'(t-1)) )
// depends on ONE score of the previous observation: position p-1's.  The pipelined plan
// (pipe_kernel.h) gives a wave a block of positions and hands the block's last score to the next
// wave every observation -- a chain of 19 waves whose exchange and fill cost a third of its time
// (DESIGN.md 5k).  Here a lane follows an anti-diagonal instead: lane l of range r holds, after
// step i, position p = (64 r + l + i) mod NP (NP = 64 x ranges >= light rows; positions past the
// last light row are +inf dummies), so the score it needs, v_{p-1}(t-1), is its own previous value.
// No lane ever reads another lane's score: no exchange, no fill, no inter-wave wait.
// Position 0 has no chain term (eb_0 = +inf), so a lane wrapping from NP-1 to 0 starts a fresh
// diagonal from F' alone, exactly as the recurrence does.
//
// What each step needs besides the lane's own score:
//   * the table pair {ea_p(o_t), eb_p(o_t)} of the lane's position: a ring in LDS holds the last
//     160 table columns the workgroup's lanes walk through, for every symbol ([S][kDR + 64 mirror]
//     float2, so the 64 lanes' read is one contiguous ds_read_b64 at any ring offset); five groups of
//     32 columns, one refilled per block of 32 steps, two groups ahead of use (global loads one block
//     before their LDS writes; one s_barrier per block), so a block's last steps can read the next
//     block's first pairs ahead of time;
//   * the uniform values of o_t: per-wave streams in LDS, built one block ahead from the sequence's
//     symbols: the constants {A_F, A_S, X_FF, X_SS}, 16 bytes per step (one broadcast ds_read_b128);
//     the ring address of (o_t, step), 4 bytes per step, read four steps at a time (one
//     ds_read_b128); and, for models whose S takes a term from F (SX), X_SF likewise.
// The steps are software-pipelined: a step's constants are read kPS steps, its ring address eight to
// eleven steps and its ring pair kPE steps before their use, across block boundaries too; the reads
// of two steps are issued together, so that one counted wait serves both.
// A workgroup is W sequences x one range of 64 diagonals: its waves walk the same ring columns
// (shared ring), each with its own sequence's symbols.
// Per step and lane (wave64):  Y = {x, x} + {A_F, A_S};  W = {F, F} + {X_FF, X_SF};
//   Z = {ea, eb} + {F, x};  x' = min(Z.eb, Z.ea);  c' = min(fl(X_SS + c), Y.A_S, W.X_SF);
//   EXEC &= ![Y.A_F < W.X_FF];  F' = W.X_FF
// -- two v_pk_add_f32 (three with SX), five VALU more (an address add among them; the check is one
// v_cmpx: a lane that fails it switches itself off until the block's end, where the wave notes which
// lanes are left) and 2.25 LDS reads (2.5 with SX).  The sink S and the violation check are
// lane-local exactly as in pipe_kernel.h (S(t) = min over lanes of a per-lane recurrence driven by
// the lane's own scores: fl(a + .) is monotone; the lane holding the S(0) chain is range 0's lane 0).
// F' is computed by every wave redundantly (the same operations: bit-identical).
// The last wave of a sequence to finish combines the ranges' partials (S, argmin, violation); a
// row whose check failed is re-run exactly by that wave's workgroup (pipe_rerun_row) in the same
// launch.
// Decoded paths of models created with SVH_KERNEL_DIAG run the PATHS instantiations of the same
// kernel (below; the record layouts are in kernels.h, the walk in pipe_paths.hip).
#include "pipe_kernel.h"

#include <algorithm>
#include <cstdlib>

namespace svh {

namespace {

#ifndef SVH_DIAG_K
#define SVH_DIAG_K 64
#endif
constexpr uint32_t kDK = SVH_DIAG_K;  // steps per block (= columns per ring group; 32 or 64)
static_assert(kDK == 32 || kDK == 64, "block length");
constexpr uint32_t kDR = 5 * kDK;     // ring columns (five groups of kDK)
constexpr uint32_t kDRS = kDR + 64;   // slots per symbol plane: the ring and a mirror of its first 64
constexpr uint32_t kDRS2 = kDR + 128; // two diagonals per lane: floats per ea / eb plane (a mirror of the first 128)
static_assert(kDRS2 % 64 == 0, "the eb plane and the second diagonal lie whole multiples of 64 floats behind the lane's ea");
constexpr uint32_t kDG = kDR / kDK;   // ring groups
constexpr uint32_t kCP = kDK / 2;     // 16-byte chunks of a plane's group (two columns each)
constexpr uint32_t kDE = 4;           // floats per entry of the constants stream
constexpr uint32_t kAG = 4;           // steps per read of the address stream and of the X_SF stream
#ifndef SVH_DIAG_PS
#define SVH_DIAG_PS 6
#endif
#ifndef SVH_DIAG_PE
#define SVH_DIAG_PE 2
#endif
constexpr uint32_t kPS = SVH_DIAG_PS;  // steps a stream entry is read ahead of its use (two at a time)
constexpr uint32_t kPE = SVH_DIAG_PE;  // steps a ring pair is read ahead of its use (< kPS)
constexpr uint32_t kNS = kPS + 2;      // stream registers: entries j .. j + kPS - 1 and the two being read
constexpr uint32_t kNE = kPE + 2;      // ring-pair registers: pairs j .. j + kPE - 1 and the two being read
static_assert(kPE + 2 <= kPS && kPS % 2 == 0 && kPE % 2 == 0 && kDK % kNS == 0 && kDK % kNE == 0,
              "prefetch distances: the register slots of step j (j % kNS, j % kNE) repeat every block");
static_assert(kPE == 2 && kDK % (2 * kAG) == 0,
              "address groups: read 2 kAG steps ahead into two register slots (group % 2), which repeat every block; "
              "a group's slot is free once the pairs of its last two steps are issued (kPE = 2)");
constexpr uint32_t kDMaxSym = 32;
static_assert(kDMaxSym == kDiagSetMaxSym, "kernels.h: what the runtime admits to a set launch");
// SVH_DIAG_AB (diagnostic builds, timing only, wrong results): 1 = no stream reads in the steps
// (every step takes the block's first entry), 2 = no ring reads (the prologue's pairs), 3 = no
// barrier between blocks, 4 = no prologue table loads, 5 = no partials / combine, 6 = return at entry,
// 7 = no arrival count (the last range combines), 8 = the arrival count without the combine
#ifndef SVH_DIAG_AB
#define SVH_DIAG_AB 0
#endif
#ifndef SVH_DIAG_FINISH
#define SVH_DIAG_FINISH 0
#endif
// SVH_DIAG_PAB (diagnostic builds of the path variant, timing only, wrong paths): 1 = no decision
// bits, 2 = no ring writes and no folds (the light minima), 3 = no record stores at the blocks' ends
// (words, checkpoints, F and sink checkpoints), 4 = one exec_collect and one fold per block (the ring
// writes stay: against 2, the cost of the collects every 8 steps)
#ifndef SVH_DIAG_PAB
#define SVH_DIAG_PAB 0
#endif
// SVH_DIAG_CMPX2 (A/B of the two-diagonal step's check): 1 = v_cmpx as everywhere else, 0 = a compare
// and an add with carry into a per-lane count, read at the row's end
#ifndef SVH_DIAG_CMPX2
#define SVH_DIAG_CMPX2 1
#endif
// SVH_DIAG_LDPRIO (A/B of the loader-wave variant): the step waves' s_setprio level, 0 = none (as
// measured: raising them costs 3 % at 50 sequences and nothing at 13)
#ifndef SVH_DIAG_LDPRIO
#define SVH_DIAG_LDPRIO 0
#endif
// SVH_DIAG_LDDRAIN (A/B of the loader-wave variant): 1 = the step waves wait for their LDS reads
// (lgkmcnt(0)) ahead of the block's barrier as the plain variant does, 0 = they do not
#ifndef SVH_DIAG_LDDRAIN
#define SVH_DIAG_LDDRAIN 1
#endif
// SVH_DIAG_QDMA (A/B of the quad ring's refill): 1 = one LDS-DMA instruction per symbol and group
// (global_load_lds_dwordx4), 0 = a global load into registers and a 16-byte LDS write per symbol
#ifndef SVH_DIAG_QDMA
#define SVH_DIAG_QDMA 1
#endif
#ifndef SVH_DIAG_DONE_STRIDE  // words between rows' arrival counts (the scratch holds 32 per row)
#define SVH_DIAG_DONE_STRIDE 1
#endif

__device__ __forceinline__ f2 lds_ld2(uint32_t a) {
    return *(const __attribute__((address_space(3))) f2*)(size_t)a;
}
__device__ __forceinline__ float lds_ld1(uint32_t a) {
    return *(const __attribute__((address_space(3))) float*)(size_t)a;
}
typedef float f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f4 lds_ld4(uint32_t a) {
    return *(const __attribute__((address_space(3))) f4*)(size_t)a;
}

// The speculation check, one VALU: EXEC &= !(a < b) (v_cmpx writes VCC and EXEC).  A lane whose
// check fails switches itself off and stays off until its wave's next exec_collect(): what it
// would have computed is never used, its row is re-run exactly (pipe_rerun_row overwrites every
// score of the row), so only the fact that it failed has to survive.  !(a < b) keeps a lane on
// where a or b is a NaN, as [a < b] counted nothing there.
// EXEC is not in the clobber list: the compiler reserves it, rejects it there with a warning and
// keeps nothing in it across straight-line code; the steps between two exec_collect() calls are
// straight-line code or a wave-uniform loop (scalar branches), and the scheduler is fenced off at
// both ends (sched_barrier), so that no lane-wise work of the all-lanes code around them (the
// cooperative ring refill above all) lands among instructions that some lanes skip.
__device__ __forceinline__ void check_off(float a, float b) {
    asm volatile("v_cmpx_nlt_f32_e32 vcc, %0, %1" : : "v"(a), "v"(b) : "vcc");
}
// alive &= EXEC; EXEC = all lanes.  s_nop 4: five wait states between a write of EXEC and a DPP
// operation (the epilogue's reductions; the compiler does not see this write).
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

__host__ __device__ constexpr size_t diag_lds_main(uint32_t W, uint32_t S, bool sx, uint32_t dm = 1, bool ld = false,
                                                   bool quad = false) {
    // ring [S][kDRS] float2 (dm = 2: [S][2][kDRS2] floats; quad: [S][kDRS] float4) | symbol template [S][8] |
    // constants [W][2][kDK][kDE] | ring addresses [W][2][kDK] | X_SF [W][2][kDK] (sx only) | blocks [W] | rerun rows [W]
    // (ld, the loader-wave variant: three stream buffers instead of two)
    return ((size_t)S * (quad ? kDRS * 2 : dm == 2 ? kDRS2 : kDRS) * 2 + (size_t)S * 8 + (size_t)W * (ld ? 3 : 2) * kDK * (kDE + 1 + (sx ? 1 : 0)) + 2 * W) * 4;
}

// Decoded paths (PATHS; the walk is pipe_paths.hip's diag entry): fold ring [W][kFS][64] floats behind
// the scores variant's LDS, 16-byte aligned.
constexpr uint32_t kFS = 8;  // steps between two folds of a wave's scores into mu partials
static_assert(kDK % kFS == 0 && 32 % kFS == 0 && kFS * 8 == 64, "fold: lane l reduces 8 lanes of step l / 8");
__host__ __device__ constexpr size_t diag_lds_paths(uint32_t W, uint32_t S, bool sx) {
    return ((diag_lds_main(W, S, sx) + 15) & ~(size_t)15) + (size_t)W * kFS * 64 * 4;
}

// PATHS: the step also records what the path walk reads (kernels.h, "Diagonal plan, decoded paths"):
// a decision bit per step, shifted into a word per lane (one compare, one add with carry), the
// lane's score into the wave's fold ring (one ds_write_b32); every kFS steps the wave folds the ring
// into the range's light minima; every 32 observations it keeps the lane's score and {F, c} for the
// block's end, where the words, the checkpoints and the range's sink partial are stored.  All of that
// all-lanes work follows an exec_collect() of its own (one per kFS steps): no lane is off in it.
// Begin is 0 for every row; a row whose check failed is not re-run here (its path needs the chain
// kernel's records: the host's fallback launch takes it, x.viol).
//
// DM = 2 (scores only): two diagonals per lane.  Lane l of range r (128 wide: NR = nrng2, NP = 128 NR
// = P) holds diagonals 128 r + l and 128 r + 64 + l, so a wave pays the step's per-wave part -- the
// constants read, the address add, the check, the {F, c} advance, the sink minimum, the scalar work
// and the wait -- once for 128 positions.  The check and the sink take m = min(x_a, x_b): fl(a + .)
// is monotone, so fl(A_F + m) < F' iff it holds for one of the two positions, and the per-lane sink
// recurrence driven by m still has the row's S as its minimum over lanes (the argument above over a
// coarser partition of the positions).  The ring holds an ea and an eb plane per symbol
// ([S][2][kDRS2] floats, a mirror of the first 128 columns behind the ring), so that one two-address
// read per plane yields {ea_a, ea_b} / {eb_a, eb_b} as register pairs and the chain and feeder
// terms are one packed add each; the lanes of a block walk through four ring groups instead of
// three, which the five groups still hold (group kb + 4 is written over group kb - 1).
//
// LD (scores only): a loader wave.  The workgroup is W step waves and one wave more (wave W), which
// does everything of a block that is not steps -- the ring refill of group kb + 4 for every symbol
// plane and the three streams of all W sequences with their symbol loads -- and meets the step
// waves at the one barrier per block; the step waves run block() / tail(), exec_collect and that
// barrier only.  A stream built by another wave is ordered by the barrier alone, so the loader
// builds block kb + 2 during block kb, into one of three buffers ("Loader wave").
// After the last block the loader wave ends: the epilogue's barriers (and pipe_rerun_row's, written
// for 64 W threads) then wait for the step waves only -- S_BARRIER: "If some waves in the
// work-group have already terminated, this waits on only the surviving waves" (AMD Instinct CDNA3 /
// CDNA4 ISA reference guides, SOPP instructions).
//
// QD (DM = 2 with LD, scores only): the quad ring.  Ring column u holds the four table values a lane
// needs of a step as one 16-byte entry {ea[c], ea[c + 64], eb[c], eb[c + 64]} (c = the column's table
// position, + 64 modulo NP: PipeModel::dtab4 holds them so), [S][kDRS] float4 -- the one-diagonal
// kernel's geometry again, five groups of 64 columns and a mirror of the first 64, three groups in use
// per block -- so a step's table read is one ds_read_b128 whose registers are the two aligned pairs
// the packed adds take, and a symbol's group is 1 KiB contiguous in the table and in the ring: the
// loader wave refills it with one global_load_lds_dwordx4 (diag_body.h, "Quad ring timing").
//
// The body is diag_body.h, included here and in diag_set_kernel below.
template <int W, bool SX, bool PATHS = false, int DM = 1, bool LD = false, bool FL = false, bool QD = false>
__global__ __launch_bounds__(64 * (W + (LD ? 1 : 0))) __attribute__((amdgpu_waves_per_eu(2)))
void diag_viterbi_kernel(PipeModel m, FusedBatch b, PipeScratch x) {
    const uint32_t bx = blockIdx.x;
#include "diag_body.h"
}

// Model sets (kernels.h DiagSetEntry): the grid is the concatenation of the entries' own grids, entry
// i's blocks being [first[i], first[i + 1]).  A workgroup's entry is the last i with first[i] <=
// blockIdx.x (first[] ascends strictly from first[0] = 0): lane l of every wave compares first[64 c + l]
// chunk by chunk, a ballot's population count is the chunk's share of the entries at or below the
// block, and the first chunk that is not all below ends the search.  The index is wave-uniform, so the
// entry's descriptor is read with scalar loads as the plain kernel's arguments are; then the plan's
// body (diag_body.h) runs as block blockIdx.x - first[i] of that entry's own launch, with that entry's
// m, b and x everywhere (partials, arrival counts, the re-run).  Workgroups of different entries share
// nothing: no wait, no spin, no communication is added.
//
// A pointer read from the descriptor table is device memory.  The compiler knows that of a kernel's
// own pointer arguments and not of a pointer it loaded: said so here (the global pointer goes through
// an empty asm statement, so that the cast pair is not folded away), the body's accesses are global
// loads and stores from scalar bases as in the plain kernel, not flat ones, which count against the
// steps' LDS waits as well.  (The descriptor is wave-uniform: "s".)
template <class T>
__device__ __forceinline__ void in_global1(T*& p) {
    auto g = (__attribute__((address_space(1))) T*)p;
    asm volatile("" : "+s"(g));
    p = (T*)g;
}
template <class... T>
__device__ __forceinline__ void in_global(T*&... p) {
    (in_global1(p), ...);
}
template <int W>
__global__ __launch_bounds__(64 * W) __attribute__((amdgpu_waves_per_eu(2)))
void diag_set_kernel(const DiagSetEntry* __restrict__ e, const uint32_t* __restrict__ first, uint32_t ne) {
    constexpr bool SX = false, PATHS = false, LD = false, FL = false, QD = false;
    constexpr int DM = 1;
    const uint32_t lane = threadIdx.x & 63u, gbx = blockIdx.x;
    uint32_t cnt = 0;
    for (uint32_t i0 = 0; i0 < ne; i0 += 64) {
        const uint32_t i = i0 + lane;
        const bool le = i < ne && first[i] <= gbx;
        const uint32_t c = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(le));
        cnt += c;
        if (c < 64) break;
    }
    if (cnt == 0) return;  // (first[0] = 0: every block has an entry)
    const uint32_t i = (uint32_t)uniform((int)(cnt - 1));
    const uint32_t f0 = first[i];
    DiagSetEntry ent = e[i];
    in_global(ent.m.tab, ent.m.e0, ent.m.start, ent.m.lrow, ent.m.hc, ent.m.dtab, ent.m.pflags, ent.m.spos, ent.m.stamps, ent.m.dtab2,
              ent.m.dtab4);
    in_global(ent.b.symbols, ent.b.sym_off, ent.b.begin, ent.b.end, ent.b.v_in, ent.b.v_in_row, ent.b.scores, ent.b.best,
              ent.b.run_mask, ent.b.fault);
    in_global(ent.x.ctr, ent.x.done, ent.x.part, ent.x.gran, ent.x.cons, ent.x.viol, ent.x.xcc);
    const PipeModel& m = ent.m;
    const FusedBatch& b = ent.b;
    const PipeScratch& x = ent.x;
    const uint32_t bx = gbx - f0;
    {
#include "diag_body.h"
    }
}

// One workgroup per row after the main launch: the row's NR partials -> S, best state, the
// violation flag; a row whose speculation failed is re-run here exactly (pipe_rerun_row).
template <bool SX>
__global__ __launch_bounds__(256) void diag_finish_kernel(PipeModel m, FusedBatch b, PipeScratch x) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u;
    uint32_t* flag = reinterpret_cast<uint32_t*>(lds + 2 * (size_t)m.P + 8);
    if (tid < 64) {
        float C = kInf, bv = kInf;
        uint32_t bk = kNoRow, vi = 0;
        for (uint32_t u = lane; u < m.nrng; u += 64) {
            const uint64_t* pu = x.part + ((size_t)q * x.G + u) * 2;
            const uint64_t a = pu[0], k2 = pu[1];
            C = fminf(C, __builtin_bit_cast(float, (uint32_t)a));
            vi |= (uint32_t)(a >> 32);
            if (k2 != ~0ull) lex_min(bv, bk, lex_key_value(k2), lex_key_index(k2));
        }
        C = wave_min63(C);
        wave_lexmin63(bv, bk);
        const bool any = __builtin_amdgcn_ballot_w64(vi != 0) != 0;
        if (lane == 63) {
            float* out = b.scores + (size_t)q * m.n;
            if (m.rowF >= 0) lex_min(bv, bk, out[m.rowF], (uint32_t)m.rowF);
            if (m.rowS >= 0) {
                out[m.rowS] = C;
                lex_min(bv, bk, C, (uint32_t)m.rowS);
            }
            if (b.best) b.best[q] = bk == kNoRow ? -1 : (int64_t)bk;
            x.viol[q] = any ? 1u : 0u;
            *flag = any ? 1u : 0u;
        }
    }
    __syncthreads();
    if (*flag) pipe_rerun_row<2, 4, SX>(m, b, q, lds);
}

template <int W, int DM = 1>
const void* diag_ptr(bool sx) {
    return sx ? reinterpret_cast<const void*>(&diag_viterbi_kernel<W, true, false, DM>)
              : reinterpret_cast<const void*>(&diag_viterbi_kernel<W, false, false, DM>);
}
template <int W, int DM>
const void* diag_loader_ptr(bool sx) {
    if constexpr (SVH_DIAG_AB != 0 || SVH_DIAG_FINISH != 0) {  // (diagnostic builds keep the plain variant: diag_loader_for)
        return nullptr;
    } else {
        return sx ? reinterpret_cast<const void*>(&diag_viterbi_kernel<W, true, false, DM, true>)
                  : reinterpret_cast<const void*>(&diag_viterbi_kernel<W, false, false, DM, true>);
    }
}
template <int W>
const void* diag_quad_ptr(bool sx) {
    if constexpr (SVH_DIAG_AB != 0 || SVH_DIAG_FINISH != 0 || kDK != 64) {
        return nullptr;
    } else {
        return sx ? reinterpret_cast<const void*>(&diag_viterbi_kernel<W, true, false, 2, true, false, true>)
                  : reinterpret_cast<const void*>(&diag_viterbi_kernel<W, false, false, 2, true, false, true>);
    }
}
// (Only the instantiations without X_SF: with both PATHS and SX the block's body is past the
// compiler's limit for `#pragma unroll`, the 64 steps are then unrolled in part, the register
// vectors indexed at run time, and the kernel is some 600 instructions per step.  Models whose S
// takes a term from F keep the chain path variant: diag_paths_fit.)
// (the floor: workgroups of four sequences only)
template <int DM>
const void* diag_floor_ptr(bool sx) {
    if constexpr (SVH_DIAG_AB != 0 || SVH_DIAG_FINISH != 0) {
        return nullptr;
    } else {
        return sx ? reinterpret_cast<const void*>(&diag_viterbi_kernel<4, true, false, DM, true, true>)
                  : reinterpret_cast<const void*>(&diag_viterbi_kernel<4, false, false, DM, true, true>);
    }
}
template <int W>
const void* diag_paths_ptr() {
    static_assert(kDK == 64, "the path records' block layout (two mask words, two checkpoints per block)");
    return reinterpret_cast<const void*>(&diag_viterbi_kernel<W, false, true>);
}

}  // namespace

uint32_t diag_waves_for(uint64_t nseq) { return nseq >= 4 ? 4u : nseq >= 2 ? 2u : 1u; }

static size_t diag_lds(uint32_t W, uint32_t S, uint32_t P, bool sx, uint32_t dm = 1, bool ld = false, bool quad = false) {
    const size_t rerun = (2 * (size_t)P + 2 * W) * 4;  // pipe_rerun_row: v[2][P], red[2][W]
    const size_t mainb = diag_lds_main(W, S, sx, dm, ld, quad);
    return mainb > rerun ? mainb : rerun;
}

// (the larger of the two kernels': models that use X_SF keep one stream more)
size_t diag_lds_bytes(uint32_t W, uint32_t S, uint32_t P, uint32_t dm, bool ld, bool quad) {
    return diag_lds(W, S, P, true, dm, ld, quad);
}

uint32_t diag_sm_for(const PipeModel& m, uint64_t nseq, bool resumed, bool paths) {
    if (paths || !m.dtab2 || !m.nrng2 || SVH_DIAG_AB != 0 || SVH_DIAG_FINISH != 0) return 1;
    if (m.dsm == 1 || m.dsm == 2) return m.dsm;
    if (resumed || !m.cus) return 1;
    const uint64_t W = diag_waves_for(nseq);
    return (nseq + W - 1) / W * W * m.nrng > 4ull * m.cus ? 2 : 1;
}

bool diag_loader_for(const PipeModel& m, uint64_t nseq, bool resumed, bool paths) {
    if (paths || !nseq || SVH_DIAG_AB != 0 || SVH_DIAG_FINISH != 0 || m.dld == 1) return false;  // (dld: kernels.h)
    const uint32_t W = diag_waves_for(nseq);
    const uint32_t dm = diag_sm_for(m, nseq, resumed, paths);
    if (diag_lds(W, m.S, m.P, m.sx != 0, dm, true) > 160 * 1024) return false;
    if (m.dld == 3) return W == 4;  // (the floor variant: svh_batch_step_floor_ms)
    if (m.dld == 2) return true;
    // a wave alone on its SIMD has no neighbour to hide the block's other work behind, and the third
    // stream buffer costs no residency: launches of at most one workgroup per CU
    return m.cus && (nseq + W - 1) / W * (dm == 2 ? m.nrng2 : m.nrng) <= m.cus;
}

bool diag_quad_table_fits(uint32_t S, uint32_t P, bool sx) {
    return SVH_DIAG_AB == 0 && SVH_DIAG_FINISH == 0 && kDK == 64 && diag_lds(1, S, P, sx, 2, true, true) <= 160 * 1024;
}

bool diag_quad_for(const PipeModel& m, uint64_t nseq, bool resumed, bool paths) {
    if (!m.dtab4 || m.dqd == 1 || m.dld == 3 || SVH_DIAG_AB != 0 || SVH_DIAG_FINISH != 0 || kDK != 64) return false;
    if (diag_sm_for(m, nseq, resumed, paths) != 2 || !diag_loader_for(m, nseq, resumed, paths)) return false;
    return diag_lds(diag_waves_for(nseq), m.S, m.P, m.sx != 0, 2, true, true) <= 160 * 1024;
}

size_t diag_paths_lds_bytes(uint32_t W, uint32_t S, bool sx) { return diag_lds_paths(W, S, sx); }

// The path variant keeps two workgroups on a CU at every width (the headline's 494 workgroups need
// them on 256 CUs): a model whose LDS does not allow that is not planned on it; nor is one whose S
// takes a term from F (sx: no such instantiation, see diag_paths_ptr).
bool diag_paths_fit(uint32_t S, bool sx) {
    return !sx && SVH_DIAG_AB == 0 && SVH_DIAG_FINISH == 0 && kDK == 64 && S > 0 && S <= kDMaxSym &&
           diag_lds_paths(4, S, sx) <= kDiagPathsLdsMax;
}

hipError_t launch_diag(const PipeModel& m, const FusedBatch& b, const PipeScratch& x, hipStream_t stream) {
    const bool paths = b.cmask != nullptr;
    if (!m.dtab || m.nrng == 0 || m.SM != 2 || m.S == 0 || m.S > kDMaxSym || (size_t)m.nrng * 64 > m.P || m.wide ||
        b.run_mask || (b.v_in && !b.v_in_row) || !x.part || !x.done || !x.viol || b.nseq > x.rows || x.G < m.nrng)
        return hipErrorInvalidValue;
    // decoded paths: every record buffer, every row from observation 0, F winning every tie (one
    // compare per decision bit), two workgroups per CU
    if (paths && (!b.cmask_off || !b.ckpt || !b.ckpt_off || !b.fck || !b.fck_off || !b.hrec || !b.hrec_off || !b.prec ||
                  !b.prec_off || b.v_in || !m.ties_heavy || !diag_paths_fit(m.S, m.sx != 0)))
        return hipErrorInvalidValue;
    if (b.nseq == 0) return hipSuccess;
    const uint32_t W = diag_waves_for(b.nseq);
    const uint32_t dm = diag_sm_for(m, b.nseq, b.v_in != nullptr, paths);
    if (dm == 2 && ((size_t)m.nrng2 * 128 != m.P || x.G < m.nrng2)) return hipErrorInvalidValue;
    const bool sx = m.sx != 0;
    const bool ld = diag_loader_for(m, b.nseq, b.v_in != nullptr, paths);
    const bool quad = diag_quad_for(m, b.nseq, b.v_in != nullptr, paths);
    const void* fn = paths     ? (W == 4 ? diag_paths_ptr<4>() : W == 2 ? diag_paths_ptr<2>() : diag_paths_ptr<1>())
                     : ld && m.dld == 3 ? (dm == 2 ? diag_floor_ptr<2>(sx) : diag_floor_ptr<1>(sx))
                     : quad    ? (W == 4 ? diag_quad_ptr<4>(sx) : W == 2 ? diag_quad_ptr<2>(sx) : diag_quad_ptr<1>(sx))
                     : ld      ? (dm == 2 ? (W == 4 ? diag_loader_ptr<4, 2>(sx) : W == 2 ? diag_loader_ptr<2, 2>(sx) : diag_loader_ptr<1, 2>(sx))
                                          : (W == 4 ? diag_loader_ptr<4, 1>(sx) : W == 2 ? diag_loader_ptr<2, 1>(sx) : diag_loader_ptr<1, 1>(sx)))
                     : dm == 2 ? (W == 4 ? diag_ptr<4, 2>(sx) : W == 2 ? diag_ptr<2, 2>(sx) : diag_ptr<1, 2>(sx))
                               : (W == 4 ? diag_ptr<4>(sx) : W == 2 ? diag_ptr<2>(sx) : diag_ptr<1>(sx));
    size_t lds = paths ? diag_lds_paths(W, m.S, sx) : diag_lds(W, m.S, m.P, sx, dm, ld, quad);
    if (lds > 160 * 1024 || !fn) return hipErrorInvalidValue;
    const uint64_t grid = ((uint64_t)b.nseq + W - 1) / W * (dm == 2 ? m.nrng2 : m.nrng);
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    // even placement: a launch that fits the chip gets its LDS request raised so that no CU can take
    // more than ceil(grid / CUs) of its workgroups (the dispatcher would otherwise stack up to four
    // on some CUs and leave others empty; the kernel ends with its most loaded CU)
    if (m.cus) {
        const uint64_t per_cu = (grid + m.cus - 1) / m.cus;
        if (per_cu * lds <= 160 * 1024) {
            const size_t cap = (160 * 1024 / per_cu) & ~(size_t)511;
            lds = cap > lds ? cap : lds;
        }
    }
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    PipeModel mm = m;
    FusedBatch bb = b;
    PipeScratch xx = x;
    void* args[] = {&mm, &bb, &xx};
    const hipError_t e = hipLaunchKernel(fn, dim3((uint32_t)grid), dim3(64 * (W + (ld ? 1 : 0))), args, lds, stream);
#if SVH_DIAG_FINISH
    if (e != hipSuccess) return e;
    const void* fin = m.sx ? reinterpret_cast<const void*>(&diag_finish_kernel<true>)
                           : reinterpret_cast<const void*>(&diag_finish_kernel<false>);
    return hipLaunchKernel(fin, dim3(b.nseq), dim3(256), args, (2 * (size_t)m.P + 8 + 1) * 4, stream);
#else
    return e;
#endif
}

hipError_t diag_set_plan(const DiagSetEntry* host, const uint32_t* first_host, uint32_t ne, DiagSetLaunch* out) {
    if (!host || !first_host || !out || ne == 0 || first_host[0] != 0 || SVH_DIAG_AB != 0 || SVH_DIAG_FINISH != 0)
        return hipErrorInvalidValue;
    const uint32_t nseq = host[0].b.nseq;
    if (nseq == 0) return hipErrorInvalidValue;
    const uint32_t W = diag_waves_for(nseq);
    size_t lds = 0;
    for (uint32_t i = 0; i < ne; ++i) {
        const PipeModel& m = host[i].m;
        const FusedBatch& b = host[i].b;
        const PipeScratch& x = host[i].x;
        // launch_diag's conditions for a scores launch, and the set's own: no X_SF term, one W
        if (!m.dtab || m.nrng == 0 || m.SM != 2 || m.S == 0 || m.S > kDMaxSym || (size_t)m.nrng * 64 > m.P || m.wide ||
            m.sx || b.run_mask || b.cmask || (b.v_in && !b.v_in_row) || !x.part || !x.done || !x.viol || b.nseq != nseq ||
            b.nseq > x.rows || x.G < m.nrng || !b.symbols || !b.sym_off || !b.begin || !b.end || !b.scores)
            return hipErrorInvalidValue;
        const uint64_t blocks = ((uint64_t)nseq + W - 1) / W * m.nrng;
        if (first_host[i + 1] < first_host[i] || (uint64_t)first_host[i + 1] - first_host[i] != blocks) return hipErrorInvalidValue;
        lds = std::max(lds, diag_lds(W, m.S, m.P, false));
    }
    if (first_host[ne] > 0x7FFFFFFFu || lds > 160 * 1024) return hipErrorInvalidValue;
    out->grid = first_host[ne];
    out->lds_bytes = lds;
    out->waves = W;
    return hipSuccess;
}

hipError_t launch_diag_set(const DiagSetEntry* host, const uint32_t* first_host, uint32_t ne, const DiagSetEntry* entries,
                           const uint32_t* first, uint32_t cus, hipStream_t stream) {
    DiagSetLaunch L{};
    const hipError_t pe = diag_set_plan(host, first_host, ne, &L);
    if (pe != hipSuccess) return pe;
    if (!entries || !first) return hipErrorInvalidValue;
    const void* fn = L.waves == 4   ? reinterpret_cast<const void*>(&diag_set_kernel<4>)
                     : L.waves == 2 ? reinterpret_cast<const void*>(&diag_set_kernel<2>)
                                    : reinterpret_cast<const void*>(&diag_set_kernel<1>);
    size_t lds = L.lds_bytes;
    // even placement over the whole grid, as launch_diag's
    if (cus) {
        const uint64_t per_cu = (L.grid + cus - 1) / cus;
        if (per_cu * lds <= 160 * 1024) {
            const size_t cap = (160 * 1024 / per_cu) & ~(size_t)511;
            lds = cap > lds ? cap : lds;
        }
    }
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const DiagSetEntry* ea = entries;
    const uint32_t* fa = first;
    uint32_t na = ne;
    void* args[] = {&ea, &fa, &na};
    return hipLaunchKernel(fn, dim3((uint32_t)L.grid), dim3(64 * L.waves), args, lds, stream);
}

}  // namespace svh
