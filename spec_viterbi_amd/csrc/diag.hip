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
constexpr uint32_t kDMaxSym = kDiagMaxSym;
// SVH_DIAG_AB (diagnostic builds, timing only, wrong results): 1 = no stream reads in the steps
// (every step takes the block's first entry), 2 = no ring reads (the prologue's pairs), 3 = no
// barrier between blocks, 4 = no prologue table loads, 5 = no partials / combine, 6 = return at entry,
// 7 = no arrival count (the last range combines), 8 = the arrival count without the combine
#ifndef SVH_DIAG_AB
#define SVH_DIAG_AB 0
#endif
// SVH_DIAG_PAB (diagnostic builds of the path variant, timing only, wrong paths): 1 = no decision
// bits, 2 = no ring writes and no folds (the light minima), 3 = no record stores at the blocks' ends
// (words, checkpoints, F and sink checkpoints), 4 = one exec_collect and one fold per block (the ring
// writes stay: against 2, the cost of the collects every 8 steps)
#ifndef SVH_DIAG_PAB
#define SVH_DIAG_PAB 0
#endif
// SVH_DIAG_RDPLACE (A/B of the quad-ring kernels' two-step body, diag_body.h block()): 0 = the order
// of every other instantiation, the body's reads at its top with the quads' address adds among them
// (in the bodies that read an address group), constants six steps ahead, quads two; 1 (the default,
// -4 %: DESIGN.md 5l, "Read placement") = both address adds ahead of the reads in every body, so that
// the two constants, the two quads and the group read issue in one run, and the constants two steps
// ahead like the quads
#ifndef SVH_DIAG_RDPLACE
#define SVH_DIAG_RDPLACE 1
#endif
// SVH_DIAG_S2PAIR (A/B of the two-diagonal step's {F, c} pair, diag_body.h step2): 0 = the pair's
// packed add and the sink's minimum as plain C++; the compiler then puts the minimum into another
// register and moves F' beside it, one v_mov_b32 per step; 1 (the default, -2 %: DESIGN.md 5l, "The
// two-diagonal step without its move") = both in one asm statement that advances the pair in place in a
// fixed register pair (v[94:95]), no move
#ifndef SVH_DIAG_S2PAIR
#define SVH_DIAG_S2PAIR 1
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

// The LDS layouts are diag_launch.h's (host and device share them); the path variant's fold ring lies
// behind this build's plain layout (diag_body.h).
constexpr size_t diag_lds_main(uint32_t W, uint32_t S, bool sx) { return svh::diag_lds_main(kDK, W, S, sx, 1, false, false); }

// Decoded paths (PATHS; the walk is pipe_paths.hip's diag entry): fold ring [W][kFS][64] floats behind
// the scores variant's LDS, 16-byte aligned.
constexpr uint32_t kFS = kDiagFoldSteps;  // steps between two folds of a wave's scores into mu partials
static_assert(kDK % kFS == 0 && 32 % kFS == 0 && kFS * 8 == 64, "fold: lane l reduces 8 lanes of step l / 8");

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
// A pointer read from the descriptor table is device memory: every one the body uses goes through
// in_global (device_common.h), so that its accesses are global loads and stores from scalar bases as in
// the plain kernel, not flat ones, which count against the steps' LDS waits as well.
// The lookup and the descriptor are diag_set_entry.h, text shared with the path variant below.
template <int W>
__global__ __launch_bounds__(64 * W) __attribute__((amdgpu_waves_per_eu(2)))
void diag_set_kernel(const DiagSetEntry* __restrict__ e, const uint32_t* __restrict__ first, uint32_t ne) {
    constexpr bool SX = false, PATHS = false, LD = false, FL = false, QD = false;
    constexpr int DM = 1;
#include "diag_set_entry.h"
    {
#include "diag_body.h"
    }
}

// The decode pass of a set (BatchSet::decode): the same lookup, the body's path variant.  The entries'
// batches -- each member's chosen rows -- differ in their sequence counts; entry i's grid is its own
// launch's at this W (an entry with fewer rows than W has idle waves, as the last group of a
// stand-alone launch has).  The record pointers and their offset tables go through in_global with the
// others.  Rows whose speculation fails are flagged in the entry's own x.viol and left to the host's
// chain launch for that entry; nothing is re-run here.
template <int W>
__global__ __launch_bounds__(64 * W) __attribute__((amdgpu_waves_per_eu(2)))
void diag_set_paths_kernel(const DiagSetEntry* __restrict__ e, const uint32_t* __restrict__ first, uint32_t ne) {
    constexpr bool SX = false, PATHS = true, LD = false, FL = false, QD = false;
    constexpr int DM = 1;
#include "diag_set_entry.h"
    {
#include "diag_body.h"
    }
}

constexpr bool kVariants = SVH_DIAG_AB == 0;  // (diagnostic builds keep the plain kernel)

template <int W, bool SX, bool PATHS = false, int DM = 1, bool LD = false, bool FL = false, bool QD = false>
const void* kernel_fn() {
    return reinterpret_cast<const void*>(&diag_viterbi_kernel<W, SX, PATHS, DM, LD, FL, QD>);
}
// The instantiation of a resolved launch; null where there is none: the floor with workgroups of four
// sequences only, the quad ring with blocks of 64 steps only, decoded paths without X_SF only (with
// both PATHS and SX the block's body is past the compiler's limit for `#pragma unroll`, the 64 steps
// are then unrolled in part, the register vectors indexed at run time, and the kernel is some 600
// instructions per step: models whose S takes a term from F keep the chain path variant).
template <int W, bool SX>
const void* diag_kernel_w(const DiagLaunch& L, bool paths) {
    if (paths) {
        static_assert(kDK == 64, "the path records' block layout (two mask words, two checkpoints per block)");
        if constexpr (!SX) return kernel_fn<W, false, true>();
        return nullptr;
    }
    if constexpr (kVariants) {
        if (L.floor) {
            if constexpr (W == 4) return L.dm == 2 ? kernel_fn<4, SX, false, 2, true, true>() : kernel_fn<4, SX, false, 1, true, true>();
            return nullptr;
        }
        if constexpr (kDK == 64)
            if (L.quad) return kernel_fn<W, SX, false, 2, true, false, true>();
        if (L.loader) return L.dm == 2 ? kernel_fn<W, SX, false, 2, true>() : kernel_fn<W, SX, false, 1, true>();
    }
    if (L.loader || L.quad || L.floor) return nullptr;
    return L.dm == 2 ? kernel_fn<W, SX, false, 2>() : kernel_fn<W, SX>();
}
const void* diag_kernel(const DiagLaunch& L, bool paths, bool sx) {
    switch (L.W) {
        case 4: return sx ? diag_kernel_w<4, true>(L, paths) : diag_kernel_w<4, false>(L, paths);
        case 2: return sx ? diag_kernel_w<2, true>(L, paths) : diag_kernel_w<2, false>(L, paths);
        case 1: return sx ? diag_kernel_w<1, true>(L, paths) : diag_kernel_w<1, false>(L, paths);
    }
    return nullptr;
}

// A (model, batch, scratch) view the scores kernel (b.cmask null) or the paths kernel takes: the
// model's shape (diag_launch.h), rows resumed with their own v_in, the scratch of this many rows and
// ranges; decoded paths: every record buffer, every row from observation 0.
bool diag_view_ok(const PipeModel& m, const FusedBatch& b, const PipeScratch& x) {
    if (!m.dtab || !diag_model_ok(diag_caps(m)) || b.run_mask || (b.v_in && !b.v_in_row) || !x.part || !x.done || !x.viol ||
        b.nseq > x.rows || x.G < m.nrng)
        return false;
    return !b.cmask || (b.cmask_off && b.ckpt && b.ckpt_off && b.fck && b.fck_off && b.hrec && b.hrec_off && b.prec && b.prec_off && !b.v_in);
}

hipError_t launch_fn(const void* fn, uint64_t grid, uint32_t threads, size_t lds, void** args, hipStream_t stream) {
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    return hipLaunchKernel(fn, dim3((uint32_t)grid), dim3(threads), args, lds, stream);
}

}  // namespace

DiagCaps diag_caps(const PipeModel& m) {
    DiagCaps c;
    c.S = m.S, c.P = m.P, c.nrng = m.nrng, c.nrng2 = m.nrng2, c.SM = m.SM, c.cus = m.cus;
    c.sx = m.sx != 0, c.wide = m.wide != 0, c.ties_heavy = m.ties_heavy != 0;
    c.dtab2 = m.dtab2 != nullptr, c.dtab4 = m.dtab4 != nullptr;
    c.dsm = m.dsm, c.dld = m.dld, c.dqd = m.dqd;
    c.dk = kDK, c.variants = kVariants;
    return c;
}

bool diag_layout_fits(uint32_t S, uint32_t P, uint32_t dm) { return diag_widest_fits(kDK, S, P, dm); }
bool diag_quad_table_fits(uint32_t S, uint32_t P, bool sx) { return diag_quad_fits(kDK, kVariants, S, P, sx); }
bool diag_paths_fit(uint32_t S, bool sx) { return svh::diag_paths_fit(kDK, kVariants, S, sx); }
bool diag_set_model_ok(const PipeModel& m) { return m.dtab && !m.sx && diag_model_ok(diag_caps(m)); }

hipError_t launch_diag(const PipeModel& m, const FusedBatch& b, const PipeScratch& x, hipStream_t stream, bool step_floor) {
    const bool paths = b.cmask != nullptr;
    if (!diag_view_ok(m, b, x)) return hipErrorInvalidValue;
    const DiagLaunch L = diag_resolve(diag_caps(m), {b.nseq, b.v_in != nullptr, paths, step_floor});
    const void* fn = diag_kernel(L, paths, m.sx != 0);
    if (!L.ok || !fn || x.G < L.ranges) return hipErrorInvalidValue;
    if (b.nseq == 0) return hipSuccess;
    PipeModel mm = m;
    FusedBatch bb = b;
    PipeScratch xx = x;
    void* args[] = {&mm, &bb, &xx};
    return launch_fn(fn, L.grid, L.threads, L.lds_request, args, stream);
}

hipError_t diag_set_plan(const DiagSetEntry* host, const uint32_t* first_host, uint32_t ne, DiagSetLaunch* out, bool paths) {
    if (!host || !first_host || !out || ne == 0 || first_host[0] != 0 || !kVariants) return hipErrorInvalidValue;
    // one W per launch: the scores entries share their sequence count; a decode's entries take what the
    // largest of them would get on its own
    uint32_t nseq = host[0].b.nseq;
    if (paths)
        for (uint32_t i = 1; i < ne; ++i) nseq = std::max(nseq, host[i].b.nseq);
    if (nseq == 0) return hipErrorInvalidValue;
    const uint32_t W = diag_resolve(diag_caps(host[0].m), {nseq, false, paths}).W;
    size_t lds = 0;
    for (uint32_t i = 0; i < ne; ++i) {
        const PipeModel& m = host[i].m;
        const FusedBatch& b = host[i].b;
        // a view launch_diag takes (scores: b.cmask null; paths: with every record buffer), and the
        // set's own conditions: no X_SF term, one W, every input
        if (!diag_view_ok(m, b, host[i].x) || !diag_set_model_ok(m) || (b.cmask != nullptr) != paths || b.nseq == 0 ||
            (!paths && b.nseq != nseq) || !b.symbols || !b.sym_off || !b.begin || !b.end || !b.scores)
            return hipErrorInvalidValue;
        if (paths && (!diag_paths_fit(m.S, false) || !m.ties_heavy)) return hipErrorInvalidValue;
        const uint64_t blocks = ((uint64_t)b.nseq + W - 1) / W * m.nrng;
        if (first_host[i + 1] < first_host[i] || (uint64_t)first_host[i + 1] - first_host[i] != blocks) return hipErrorInvalidValue;
        // (the plain variant, one diagonal per lane)
        lds = std::max(lds, paths ? diag_lds_paths(kDK, W, m.S, false) : diag_lds_scores(kDK, W, m.S, m.P, false, 1, false, false));
    }
    if (first_host[ne] > 0x7FFFFFFFu || lds > kDiagLdsMax) return hipErrorInvalidValue;
    out->grid = first_host[ne];
    out->lds_bytes = lds;
    out->waves = W;
    return hipSuccess;
}

template <int W>
const void* set_kernel_fn(bool paths) {
    static_assert(kDK == 64, "the path records' block layout (diag_kernel_w)");
    return paths ? reinterpret_cast<const void*>(&diag_set_paths_kernel<W>) : reinterpret_cast<const void*>(&diag_set_kernel<W>);
}

hipError_t launch_diag_set(const DiagSetEntry* host, const uint32_t* first_host, uint32_t ne, const DiagSetEntry* entries,
                           const uint32_t* first, uint32_t cus, hipStream_t stream, bool paths) {
    DiagSetLaunch L{};
    const hipError_t pe = diag_set_plan(host, first_host, ne, &L, paths);
    if (pe != hipSuccess) return pe;
    if (!entries || !first) return hipErrorInvalidValue;
    const void* fn = L.waves == 4 ? set_kernel_fn<4>(paths) : L.waves == 2 ? set_kernel_fn<2>(paths) : set_kernel_fn<1>(paths);
    const DiagSetEntry* ea = entries;
    const uint32_t* fa = first;
    uint32_t na = ne;
    void* args[] = {&ea, &fa, &na};
    // even placement over the whole grid
    return launch_fn(fn, L.grid, 64 * L.waves, even_placement_lds(L.grid, cus, L.lds_bytes), args, stream);
}

}  // namespace svh
