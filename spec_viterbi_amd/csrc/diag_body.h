// The body of the diagonal plan's kernels (diag.hip), included inside a kernel: one workgroup's whole
// pass.  In scope where it is included: the template parameters W, SX, PATHS, DM, LD, FL, QD (as constants
// where the kernel fixes them), the launch's `m` (PipeModel), `b` (FusedBatch), `x` (PipeScratch) and
// `bx`, the workgroup's index within that launch's grid (rg = bx % NR, grp = bx / NR).
// diag_viterbi_kernel has its arguments and blockIdx.x there; diag_set_kernel the triple and the local
// block index of the set member the workgroup belongs to.  Text, not a function: as an inlined
// function of (m, b, x, bx) the same statements compile to different code in every instantiation
// (the callee is simplified before it is inlined; 31 of 31 kernels differed), as text the existing
// instantiations are instruction for instruction what they were (tools/asm_same.py).
    static_assert(DM == 1 || (DM == 2 && !PATHS), "decoded paths keep one diagonal per lane");
    static_assert(!LD || (!PATHS && SVH_DIAG_AB == 0), "the loader wave: scores only");
    static_assert(!FL || LD, "the floor is a loader-wave launch");
    static_assert(!QD || (DM == 2 && LD && !PATHS && !FL && kDK == 64),
                  "the quad ring: two diagonals per lane, the loader wave, scores only; a group is one wave's 64 x 16 bytes");
    constexpr uint32_t NB = LD ? 3 : 2;                  // stream buffers per wave
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr uint32_t RW = 64 * DM;                     // diagonals (positions) per range
    constexpr uint32_t RS = QD ? kDRS * 2 : DM == 2 ? kDRS2 : kDRS;  // pairs of floats per symbol in the ring
    const uint32_t S = m.S, NR = DM == 2 ? m.nrng2 : m.nrng, NP = NR * RW, P = m.P;
    float* ring = lds;                                   // [S][kDRS] {ea, eb}; DM = 2: [S][2][kDRS2]; QD: [S][kDRS] quads
    float* hcr = ring + (size_t)S * RS * 2;              // [S][8] stream template of symbol o
    float* strm = hcr + S * 8;                           // [W][NB][kDK] {A_F, A_S, X_FF, X_SS}
    float* adr = strm + W * NB * kDK * kDE;              // [W][NB][kDK] ring address of (o_t, step)
    float* xsf = adr + W * NB * kDK;                     // [W][NB][kDK] X_SF (SX only)
    uint32_t* wnb = reinterpret_cast<uint32_t*>(xsf + (SX ? W * NB * kDK : 0));  // [W] blocks of wave w
    uint32_t* rrow = wnb + W;                            // [W] row wave w's combine hands to the re-run

    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t w = (uint32_t)uniform((int)(tid >> 6));
    const uint32_t rg = bx % NR, grp = bx / NR;
    const uint32_t q = grp * W + w;
    const bool ldr = LD && w == W;                        // the loader wave (wave-uniform)
    // FL (svh_batch_step_floor_ms, launched for m.dld == 3: timing only, wrong scores): the plan's
    // floor -- the prologue and the steps' arithmetic alone.  The full blocks' steps issue no LDS
    // read (every step takes the constants, the ring address and the pair the prologue read, as the
    // SVH_DIAG_AB = 1 and 2 diagnostics do); the loader wave fills group 4 and the third stream
    // buffer in the prologue (every LDS word a tail step reads is then a valid, if stale, entry) and
    // only meets the barriers; the step waves store their scores and skip the partials, the arrival
    // count, the combine and the re-run.
    constexpr bool flr = FL;
    const bool real = (!LD || w < W) && q < b.nseq;
    const uint32_t ring_a = lds_addr(ring);

    // stream template: {A_F, A_S, X_FF, X_SS, X_SF, LDS address of plane o, 0, 0}
    for (uint32_t i = tid; i < S * 8; i += 64 * (W + (LD ? 1 : 0))) {
        const uint32_t o = i >> 3, k = i & 7u;
        const float* h = m.hc + o * 8;  // A_S A_F X_SS X_FF | X_SF E_F E_S 0
        float v = 0.0f;
        if (k == 0) v = h[1];
        else if (k == 1) v = h[0];
        else if (k == 2) v = h[3];
        else if (k == 3) v = h[2];
        else if (k == 4) v = SX ? h[4] : kInf;
        else if (k == 5) v = __builtin_bit_cast(float, ring_a + o * RS * 8u);
        hcr[i] = v;
    }

    const uint8_t* __restrict__ sym = b.symbols + (real ? b.sym_off[q] : 0);
    const uint32_t len = real ? (uint32_t)uniform((int)b.end[q]) : 0u;
    const uint32_t beg = real ? (uint32_t)uniform((int)b.begin[q]) : 0u;
    const uint32_t first = beg ? beg : 1u;                // first observation the steps run (state at first-1)
    const uint32_t nst = len > first ? len - first : 0u;  // steps: observations first .. len-1
    const uint32_t nb = (nst + kDK - 1) / kDK;
    if (lane == 0 && (!LD || w < W)) {
        wnb[w] = nb;
        rrow[w] = kNoRow;
    }

    // ---- ring refill: group g = columns u in [kDK g, kDK g + kDK) of this range (table column
    // (64 rg + u) mod NP), every symbol plane; 16 chunks of 16 bytes per plane over the workgroup
    constexpr uint32_t kT = 64 * W;
    constexpr uint32_t kRep = (kCP * kDMaxSym + kT - 1) / kT;
    const uint32_t nchunk = kCP * S;
    typedef float lvec __attribute__((ext_vector_type(4 * kRep)));  // a vector, not an array: stays in VGPRs
    lvec lreg;
    auto gload = [&](uint32_t g) {
        const uint32_t c0 = (rg * RW + g * kDK) % NP;
#pragma unroll
        for (uint32_t r = 0; r < kRep; ++r) {
            // unconditional (clamped) loads: the registers stay registers
            const uint32_t k = min(tid + r * kT, nchunk - 1);
            // (DM = 2: a symbol's kCP chunks are its ea plane's kCP / 2, four columns each, then its eb plane's)
            const float4 v = DM == 2 ? *reinterpret_cast<const float4*>(m.dtab2 + (size_t)(k / (kCP / 2)) * NP + c0 + 4 * (k % (kCP / 2)))
                                     : *reinterpret_cast<const float4*>(m.dtab + (size_t)(k / kCP) * NP + c0 + 2 * (k % kCP));
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
                float* d = DM == 2 ? ring + (size_t)(k / (kCP / 2)) * kDRS2 + s0 + 4 * (k % (kCP / 2))
                                   : ring + ((size_t)(k / kCP) * kDRS + s0 + 2 * (k % kCP)) * 2;
                const float4 v = make_float4(lreg[4 * r], lreg[4 * r + 1], lreg[4 * r + 2], lreg[4 * r + 3]);
                *reinterpret_cast<float4*>(d) = v;
                if (s0 < RW) *reinterpret_cast<float4*>(d + kDR * (DM == 2 ? 1 : 2)) = v;
            }
        }
    };
    // ---- per-wave stream of block kb (steps kDK kb + 1 + j, step i reading observation first - 1 + i):
    // lane j builds entry j from the symbol it loaded one block earlier
    uint32_t symv = 0;
    auto symload = [&](uint32_t kb) {
        const uint32_t t = first + kb * kDK + lane;
        const uint32_t tc = t < len ? t : (len ? len - 1 : 0u);
        symv = (real && lane < kDK) ? (uint32_t)sym[tc] : 0u;
    };
    auto sbuild = [&](uint32_t kb) {
        if (lane < kDK) {
            const uint32_t o = symv < S ? symv : 0u;
            const float4 h0 = *reinterpret_cast<const float4*>(hcr + o * 8);
            const float2 h1 = *reinterpret_cast<const float2*>(hcr + o * 8 + 4);
            const uint32_t i = kb * kDK + 1 + lane;
            const uint32_t e = (w * 2 + (kb & 1u)) * kDK + lane;
            *reinterpret_cast<float4*>(strm + e * kDE) = h0;
            adr[e] = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, h1.y) + (i % kDR) * (DM == 2 ? 4u : 8u));
            if (SX) xsf[e] = h1.x;
        }
    };
    // ---- the loader wave's own forms of the four (LD): the refill's chunks over its 64 lanes, the
    // streams of every sequence u of the workgroup (three buffers: block kb's is kb % 3)
    constexpr uint32_t kRepL = kCP * kDMaxSym / 64;
    typedef float lvecl __attribute__((ext_vector_type(LD ? 4 * kRepL : 4)));
    lvecl lregl = 0.0f;
    const uint8_t* lsym[W] = {};
    uint32_t llen[W] = {}, lfirst[W] = {}, lsymv[W] = {};
    bool lreal[W] = {};
    auto gloadl = [&](uint32_t g) {
        if constexpr (LD) {
            const uint32_t c0 = (rg * RW + g * kDK) % NP;
#pragma unroll
            for (uint32_t r = 0; r < kRepL; ++r) {
                if (r * 64 < nchunk) {  // (wave-uniform)
                    const uint32_t k = min(lane + r * 64, nchunk - 1);
                    const float4 v = DM == 2 ? *reinterpret_cast<const float4*>(m.dtab2 + (size_t)(k / (kCP / 2)) * NP + c0 + 4 * (k % (kCP / 2)))
                                             : *reinterpret_cast<const float4*>(m.dtab + (size_t)(k / kCP) * NP + c0 + 2 * (k % kCP));
                    lregl[4 * r] = v.x;
                    lregl[4 * r + 1] = v.y;
                    lregl[4 * r + 2] = v.z;
                    lregl[4 * r + 3] = v.w;
                }
            }
        }
    };
    auto lwritel = [&](uint32_t g) {
        if constexpr (LD) {
            const uint32_t s0 = (g % kDG) * kDK;
#pragma unroll
            for (uint32_t r = 0; r < kRepL; ++r) {
                const uint32_t k = lane + r * 64;
                if (k < nchunk) {
                    float* d = DM == 2 ? ring + (size_t)(k / (kCP / 2)) * kDRS2 + s0 + 4 * (k % (kCP / 2))
                                       : ring + ((size_t)(k / kCP) * kDRS + s0 + 2 * (k % kCP)) * 2;
                    const float4 v = make_float4(lregl[4 * r], lregl[4 * r + 1], lregl[4 * r + 2], lregl[4 * r + 3]);
                    *reinterpret_cast<float4*>(d) = v;
                    if (s0 < RW) *reinterpret_cast<float4*>(d + kDR * (DM == 2 ? 1 : 2)) = v;
                }
            }
        }
    };
    auto symloadl = [&](uint32_t kb) {
#pragma unroll
        for (int u = 0; u < W; ++u) {
            const uint32_t t = lfirst[u] + kb * kDK + lane;
            const uint32_t tc = t < llen[u] ? t : (llen[u] ? llen[u] - 1 : 0u);
            lsymv[u] = (lreal[u] && lane < kDK) ? (uint32_t)lsym[u][tc] : 0u;
        }
    };
    auto sbuildl = [&](uint32_t kb) {
        if (lane < kDK) {
            const uint32_t i = kb * kDK + 1 + lane;
            const uint32_t ro = (i % kDR) * (QD ? 16u : DM == 2 ? 4u : 8u);
            const uint32_t e0 = (kb % NB) * kDK + lane;
#pragma unroll
            for (int u = 0; u < W; ++u) {
                const uint32_t o = lsymv[u] < S ? lsymv[u] : 0u;
                const float4 h0 = *reinterpret_cast<const float4*>(hcr + o * 8);
                const float2 h1 = *reinterpret_cast<const float2*>(hcr + o * 8 + 4);
                const uint32_t e = u * NB * kDK + e0;
                *reinterpret_cast<float4*>(strm + e * kDE) = h0;
                adr[e] = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, h1.y) + ro);
                if (SX) xsf[e] = h1.x;
            }
        }
    };
    // ---- the quad ring's refill (QD): group g of symbol o is 64 quads, 1 KiB contiguous in dtab4 (from
    // column c0 of the symbol's row) and in the ring (from slot s0 of the symbol's plane): one LDS-DMA
    // wave-instruction, lane l's 16 bytes from dtab4[o][c0 + l] to the wave-uniform base + 16 l; a group
    // that is the ring's first goes into the mirror behind the ring as well.  Wave wv of nw takes the
    // symbols o = wv, wv + nw, ...  Not waited for here.
    auto qfill = [&](uint32_t g, uint32_t wv, uint32_t nw) {
        if constexpr (QD) {
            const uint32_t c0 = (rg * RW + g * kDK) % NP;
            const uint32_t s0 = (g % kDG) * kDK;
            const float4* src = m.dtab4 + c0 + lane;
            for (uint32_t o = wv; o < S; o += nw) {
                const uint32_t d = ring_a + (o * kDRS + s0) * 16u;
                lds_dma16(src + (size_t)o * NP, d);
                if (s0 == 0) lds_dma16(src + (size_t)o * NP, d + kDR * 16u);
            }
        }
    };
    if constexpr (LD) {
        if (ldr) {
#pragma unroll
            for (int u = 0; u < W; ++u) {
                const uint32_t qu = grp * W + u;
                lreal[u] = qu < b.nseq;
                lsym[u] = b.symbols + (lreal[u] ? b.sym_off[qu] : 0);
                llen[u] = lreal[u] ? (uint32_t)uniform((int)b.end[qu]) : 0u;
                const uint32_t bu = lreal[u] ? (uint32_t)uniform((int)b.begin[qu]) : 0u;
                lfirst[u] = bu ? bu : 1u;
            }
        }
    }

    // ---- prologue: groups 0..3 in the ring, group 4 in flight; the stream of block 0
#if SVH_DIAG_AB == 6  // diagnostics: the launch alone
    return;
#endif
    if constexpr (LD) {
        // the step waves fill groups 0..3; the loader wave: group 4 in flight, the streams of blocks
        // 0 and 1 (behind the barrier: they need the symbol template), the symbols of block 2
        if constexpr (QD) {
            // the step waves fill groups 0..3 (the loader wave's first is group 4, during block 0); all
            // of it has landed (vmcnt(0)) in the issuing wave ahead of the first of the two barriers
            // before the first ring read
            if (ldr) {
                symloadl(0);
            } else {
                qfill(0, w, W);
                qfill(1, w, W);
                qfill(2, w, W);
                qfill(3, w, W);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else if (ldr) {
            gloadl(4);
            symloadl(0);
        } else {
            gload(0);
            lwrite(0);
            gload(1);
            lwrite(1);
            gload(2);
            lwrite(2);
            gload(3);
            lwrite(3);
        }
        __syncthreads();  // the symbol template
        if (ldr) {
            sbuildl(0);
            symloadl(1);
            sbuildl(1);
            symloadl(2);
            if (flr) {
                sbuildl(2);
                lwritel(4);
            }
        }
    } else {
#if SVH_DIAG_AB != 4  // diagnostics: no prologue table loads (rows of one observation stay exact)
    gload(0);
    lwrite(0);
    gload(1);
    lwrite(1);
    gload(2);
    lwrite(2);
    gload(3);
    lwrite(3);
    gload(4);
#endif
    symload(0);
    __syncthreads();  // the symbol template
    sbuild(0);
    symload(1);
    }

    // ---- decoded paths: this wave's record rows (lane-wise parts computed here, with every lane on)
    const uint32_t Lg = rg * 64 + lane;                   // the lane's diagonal: position (Lg + t) mod NP at observation t
    const uint32_t nck = len ? (len - 1) / kDiagCkptEvery + 1 : 0u;
    uint32_t* dmq = nullptr;                              // [word][NP] + Lg
    float *ckq = nullptr, *fckq = nullptr, *cckq = nullptr, *pmq = nullptr, *fr_wr = nullptr;
    const float* fr_rd = nullptr;
    uint32_t pcur = Lg;                                   // the lane's position at the last stored checkpoint
    if constexpr (PATHS) {
        float* fring = lds + ((diag_lds_main(W, S, SX) + 15) & ~(size_t)15) / 4 + w * kFS * 64;
        fr_wr = fring + lane;                             // step s of a fold group: + 64 s
        fr_rd = fring + lane * 8;                         // step lane / 8, lanes 8 (lane % 8) .. + 7
        if (real) {
            dmq = b.cmask + b.cmask_off[q] + Lg;
            ckq = b.ckpt + b.ckpt_off[q];
            fckq = b.fck + b.fck_off[q];
            cckq = reinterpret_cast<float*>(b.hrec + b.hrec_off[q]) + (size_t)rg * nck;
            pmq = reinterpret_cast<float*>(b.prec) + b.prec_off[q] + (size_t)rg * len + (lane >> 3);
        }
    }

    // ---- state at observation first - 1
    float xv = kInf, xv2 = kInf, F = kInf, c = kInf;  // (xv2: the lane's second diagonal, DM = 2)
    uint64_t alive = ~0ull;  // lanes whose check has held so far (collected from EXEC after every block)
    if (real && beg == 0) {
        const uint32_t o0 = (uint32_t)uniform((int)sym[0]);
        const uint32_t p = rg * RW + lane;
        xv = m.e0[(size_t)o0 * P + p] + m.start[p];
        if (DM == 2) xv2 = m.e0[(size_t)o0 * P + p + 64] + m.start[p + 64];
        F = m.rowF >= 0 ? m.hc[o0 * 8 + 5] + m.startF : kInf;
        c = (rg == 0 && lane == 0 && m.rowS >= 0) ? m.hc[o0 * 8 + 6] + m.startS : kInf;
    } else if (real) {  // resumed row (the _spec tail, time-parallel segments): scores of first-1
        const float* vin = b.v_in + (size_t)b.v_in_row[q] * m.n;
        const uint32_t r = m.lrow[rg * RW + lane];
        xv = r != kNoRow ? vin[r] : kInf;
        if (DM == 2) {
            const uint32_t r2 = m.lrow[rg * RW + 64 + lane];
            xv2 = r2 != kNoRow ? vin[r2] : kInf;
        }
        F = m.rowF >= 0 ? vin[m.rowF] : kInf;
        c = (rg == 0 && lane == 0 && m.rowS >= 0) ? vin[m.rowS] : kInf;
    }
    if constexpr (PATHS) {  // the records of observation 0
        if (real) {
            ckq[Lg] = xv;
            float mu0 = xv, c0 = c;
            wave_min63x2(mu0, c0);
            if (lane == 63) {
                pmq[-7] = mu0;  // (lane 63: pmq is the range's row + 7)
                cckq[0] = c0;
            }
            if (rg == 0 && lane == 0) fckq[0] = F;
        }
    }
    __syncthreads();  // ring groups 0..3, wnb
    uint32_t nbmax = 0;
#pragma unroll
    for (int u = 0; u < W; ++u) nbmax = wnb[u] > nbmax ? wnb[u] : nbmax;
    nbmax = (uint32_t)uniform((int)nbmax);

    // software pipeline: stream entries of steps j .. j + kPS + 1 and ring pairs of j .. j + kPE + 1
    // in registers (slot j % kNS, j % kNE)
    // (RP, SVH_DIAG_RDPLACE: the quad ring's read placement, block() below; with it the constants are
    // read two steps ahead like the quads, PS / NS in the place of kPS / kNS)
    constexpr int RP = (QD && SVH_DIAG_AB == 0) ? SVH_DIAG_RDPLACE : 0;
    constexpr uint32_t PS = RP ? kPE : kPS, NS = PS + 2;
    static_assert((RP == 0 || RP == 1) && kDK % NS == 0, "read placement; the register slots of step j repeat every block");
    typedef float hvec __attribute__((ext_vector_type(4 * NS)));
    typedef float avec __attribute__((ext_vector_type(2 * kAG)));
    typedef float evec __attribute__((ext_vector_type(2 * DM * kNE)));
    hvec hq;
    avec aq, xq;  // ring addresses / X_SF of two groups of kAG steps (slot group % 2)
    evec eq;
    // entry j of block kb in the streams' two buffers (j < 2 kDK: the next block's past kDK - 1): the
    // block's buffer or the other one (two bases per block, the rest is an immediate offset)
    // (LD: three buffers, block kb's is kb % 3)
    auto spos = [&](uint32_t kb, uint32_t j) {
        if constexpr (LD) return (w * NB + (j < kDK ? kb : kb + 1) % NB) * kDK + j % kDK;
        const uint32_t e0 = (w * 2 + (kb & 1u)) * kDK;
        return (j < kDK ? e0 : e0 ^ kDK) + j % kDK;
    };
    auto sread = [&](uint32_t kb, uint32_t j, uint32_t slot) {  // constants of step j
        const float4 h = *reinterpret_cast<const float4*>(strm + spos(kb, j) * kDE);
        hq[4 * slot] = h.x;
        hq[4 * slot + 1] = h.y;
        hq[4 * slot + 2] = h.z;
        hq[4 * slot + 3] = h.w;
    };
    auto gread = [&](avec& q, const float* src, uint32_t kb, uint32_t j) {  // steps j .. j + kAG - 1 (kAG | j)
        const float4 g = *reinterpret_cast<const float4*>(src + spos(kb, j));
        const uint32_t slot = (j / kAG) % 2;
        q[4 * slot] = g.x;
        q[4 * slot + 1] = g.y;
        q[4 * slot + 2] = g.z;
        q[4 * slot + 3] = g.w;
    };
    auto eread = [&](uint32_t j) {  // ring pair of step j (< 2 kDK)
        // (the element copied to a scalar first: __builtin_bit_cast of an ext-vector element lvalue
        // reads the vector's first element)
        const float roff = aq[j % (2 * kAG)];
        if constexpr (QD) {  // {ea_a, ea_b, eb_a, eb_b}: one 16-byte read
            const f4 e = lds_ld4(__builtin_bit_cast(uint32_t, roff) + lane * 16u);
            eq[4 * (j % kNE)] = e.x;
            eq[4 * (j % kNE) + 1] = e.y;
            eq[4 * (j % kNE) + 2] = e.z;
            eq[4 * (j % kNE) + 3] = e.w;
            return;
        }
        if constexpr (DM == 2) {  // {ea_a, ea_b}, {eb_a, eb_b}: one two-address read per plane
            const uint32_t a = __builtin_bit_cast(uint32_t, roff) + lane * 4u;
            eq[4 * (j % kNE)] = lds_ld1(a);
            eq[4 * (j % kNE) + 1] = lds_ld1(a + 256u);
            eq[4 * (j % kNE) + 2] = lds_ld1(a + kDRS2 * 4u);
            eq[4 * (j % kNE) + 3] = lds_ld1(a + kDRS2 * 4u + 256u);
            return;
        }
        const f2 e = lds_ld2(__builtin_bit_cast(uint32_t, roff) + lane * 8u);
        eq[2 * (j % kNE)] = e.x;
        eq[2 * (j % kNE) + 1] = e.y;
    };
#pragma unroll
    for (uint32_t j = 0; j < PS; ++j) sread(0, j, j);
    gread(aq, adr, 0, 0);
    gread(aq, adr, 0, kAG);
    if (SX) gread(xq, xsf, 0, 0);
#pragma unroll
    for (uint32_t j = 0; j < kPE; ++j) eread(j);

    // the state as two register pairs: {F, c} (the feeder and the lane's sink partial: one packed add
    // advances both, {X_FF + F, X_SS + c}) and {x, -} (the lane's score: the source of the packed
    // heavy terms {A_F + x, A_S + x})
    f2 FC = (f2){F, c};
    f2 XP = (f2){xv, 0.0f};
    uint32_t dw = 0;  // PATHS: the decision bits of the last 32 steps, the latest in bit 0
    auto step = [&](const float4& h, float xs, const f2& e, uint32_t slot = 0) {
        const f2 Y = XP.xx + (f2){h.x, h.y};  // {A_F + x, A_S + x}
        const f2 Wv = FC + (f2){h.z, h.w};    // {F' = X_FF + F, X_SS + c}
        const float za = e.x + FC.x;          // ea + F
        const float zb = e.y + XP.x;          // eb + x
        float cn = fminf(Wv.y, Y.y);
        if (SX) cn = fminf(cn, xs + FC.x);    // X_SF + F
        check_off(Y.x, Wv.x);                 // the speculation check: F' would have taken A_F + x
        if constexpr (PATHS && SVH_DIAG_PAB != 1) push_le(dw, za, zb);  // F's term taken (F wins every tie: ties_heavy)
        XP.x = fminf(zb, za);
        FC = (f2){Wv.x, cn};
        if constexpr (PATHS && SVH_DIAG_PAB != 2) fr_wr[slot * 64] = XP.x;
    };
    // DM = 2: the scores of the lane's two diagonals as one pair, their minimum in a pair of its own
    // (the source of the packed heavy terms)
    f2 X2 = (f2){xv, xv2};
    auto step2 = [&](const float4& h, float xs, const f2& ea, const f2& eb) {
        XP.x = fminf(X2.x, X2.y);             // m: what the check and the sink need of the two scores
        const f2 Y = XP.xx + (f2){h.x, h.y};  // {A_F + m, A_S + m}
#if SVH_DIAG_S2PAIR
        // The pair advances in place, in one fixed register pair: the packed add {X_FF + F, X_SS + c}
        // writes it, and the sink's minimum writes its second register.  Left to the compiler, the
        // minimum goes to another register and a v_mov_b32 per step puts F' beside it.
        // The same instructions on the same operands otherwise.  (The pair is read and written, and
        // marked early-clobber: no other operand of the statement may share its registers.)
        const f2 za = ea + FC.xx;             // {ea_a + F, ea_b + F}
        const f2 zb = eb + X2;                // {eb_a + x_a, eb_b + x_b}
        const f2 hzw = (f2){h.z, h.w};
        if (SX) {
            const float xf = xs + FC.x;       // X_SF + F
            asm("v_pk_add_f32 %0, %0, %1\n\tv_min3_f32 v95, v95, %2, %3" : "+&{v[94:95]}"(FC) : "v"(hzw), "v"(Y.y), "v"(xf));
        } else {
            asm("v_pk_add_f32 %0, %0, %1\n\tv_min_f32 v95, v95, %2" : "+&{v[94:95]}"(FC) : "v"(hzw), "v"(Y.y));
        }
        check_off(Y.x, FC.x);
        X2 = (f2){fminf(zb.x, za.x), fminf(zb.y, za.y)};
#else
        const f2 Wv = FC + (f2){h.z, h.w};    // {F' = X_FF + F, X_SS + c}
        const f2 za = ea + FC.xx;             // {ea_a + F, ea_b + F}
        const f2 zb = eb + X2;                // {eb_a + x_a, eb_b + x_b}
        float cn = fminf(Wv.y, Y.y);
        if (SX) cn = fminf(cn, xs + FC.x);    // X_SF + F
        check_off(Y.x, Wv.x);
        X2 = (f2){fminf(zb.x, za.x), fminf(zb.y, za.y)};
        FC = (f2){Wv.x, cn};
#endif
    };
    // PATHS, after an exec_collect: the last n <= kFS steps' scores (observations t0 .. t0 + n - 1) ->
    // the range's light minima.  Lane l takes lanes 8 (l % 8) .. + 7 of step l / 8; three DPP stages
    // join the step's 8 lanes.  In two halves: fold_read issues the lane's two ring reads, fold_min
    // reduces and stores them -- in a full block one collect later, so that the reads' latency passes
    // under the next 8 steps (the ring's slots may be rewritten meanwhile: LDS operations of a wave
    // execute in order).  The record's index and the values read go through registers defined behind
    // the collect, so that nothing lane-wise of the fold can be computed while lanes are off.
    float4 fa0 = make_float4(kInf, kInf, kInf, kInf), fa1 = fa0;
    auto fold_read = [&]() {
        if (SVH_DIAG_PAB == 2) return;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        fa0 = *reinterpret_cast<const float4*>(fr_rd);
        fa1 = *reinterpret_cast<const float4*>(fr_rd + 4);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    };
    auto fold_min = [&](uint32_t t0, uint32_t n) {
        if (SVH_DIAG_PAB == 2) return;
        uint32_t tv = t0;
        float4 a0 = fa0, a1 = fa1;
        asm volatile("" : "+v"(tv), "+v"(a0.x), "+v"(a0.y), "+v"(a0.z), "+v"(a0.w), "+v"(a1.x), "+v"(a1.y), "+v"(a1.z), "+v"(a1.w));
        float mn = fminf(fminf(fminf(a0.x, a0.y), fminf(a0.z, a0.w)), fminf(fminf(a1.x, a1.y), fminf(a1.z, a1.w)));
        const uint32_t inf = 0x7f800000u;
        mn = fminf(mn, __builtin_bit_cast(float, dpp_u<0xB1>(__builtin_bit_cast(uint32_t, mn), inf)));   // quad_perm [1,0,3,2]
        mn = fminf(mn, __builtin_bit_cast(float, dpp_u<0x4E>(__builtin_bit_cast(uint32_t, mn), inf)));   // quad_perm [2,3,0,1]
        mn = fminf(mn, __builtin_bit_cast(float, dpp_u<0x141>(__builtin_bit_cast(uint32_t, mn), inf)));  // row_half_mirror
        if ((lane & 7u) == 0 && (lane >> 3) < n) pmq[tv] = mn;  // (pmq: the range's row + lane / 8)
    };
    auto fold = [&](uint32_t t0, uint32_t n) {
        fold_read();
        fold_min(t0, n);
    };
    // PATHS: what a block keeps of its 32nd step and stores at its end
    uint32_t dw0 = 0;
    float xs0 = kInf, fs0 = kInf, cs0 = kInf;
    auto keep32 = [&]() {
        dw0 = dw;
        xs0 = XP.x;
        fs0 = FC.x;
        cs0 = FC.y;
    };
    // PATHS, after the block's last exec_collect: the records of block kb, rem of its steps run
    // (rem = kDK: dw0 / dw hold rows 64 kb .. + 31 / + 32 .. + 63; a partial word is left-aligned: row r
    // is bit 31 - r % 32); checkpoints of observations 64 kb + 32 (kept) and 64 kb + 64 (the state)
    auto block_records = [&](uint32_t kb, uint32_t rem) {
        if (SVH_DIAG_PAB == 3) {  // (the kept values stay live)
            asm volatile("" : : "v"(dw0), "v"(dw), "v"(xs0), "v"(fs0), "v"(cs0));
            return;
        }
        // (as in fold: what the stores' addresses and the DPP reduction are made of is defined here,
        // behind the collect)
        uint32_t kv = kb, pc = pcur;
        float cn1 = cs0, cn2 = FC.y;
        asm volatile("" : "+v"(kv), "+v"(pc), "+v"(cn1), "+v"(cn2));
        const uint32_t w0 = rem > 32 ? dw0 : dw << (32u - rem);
        dmq[(size_t)(2 * kv) * NP] = w0;
        if (rem > 32) dmq[(size_t)(2 * kv + 1) * NP] = dw << (64u - rem);
        if (rem >= 32) {
            const bool two = rem == 64;
            uint32_t p1 = pc + 32;
            p1 = p1 >= NP ? p1 - NP : p1;
            uint32_t p2 = p1 + 32;
            p2 = p2 >= NP ? p2 - NP : p2;
            const float x1 = rem > 32 ? xs0 : XP.x, f1 = rem > 32 ? fs0 : FC.x;
            float c1 = rem > 32 ? cn1 : cn2, c2 = cn2;
            ckq[(size_t)(2 * kv + 1) * NP + p1] = x1;
            if (two) ckq[(size_t)(2 * kv + 2) * NP + p2] = XP.x;
            wave_min63x2(c1, c2);
            if (lane == 63) {
                cckq[2 * kv + 1] = c1;
                if (two) cckq[2 * kv + 2] = c2;
            }
            if (rg == 0 && lane == 0) {
                fckq[2 * kv + 1] = f1;
                if (two) fckq[2 * kv + 2] = FC.x;
            }
            pcur = p2;
        }
    };
    auto blockwork = [&](uint32_t kb) {
        lwrite(kb + 4);  // into the slots of group kb - 1, which no wave reads any more
        gload(kb + 5);
        sbuild(kb + 1);  // into the buffer of block kb - 1 (the last steps of block kb read its first entries)
        symload(kb + 2);
    };
    auto block = [&](uint32_t kb) {
        __builtin_amdgcn_sched_barrier(0);  // the block's work stays above the first check
#pragma unroll
        for (uint32_t j = 0; j < kDK; ++j) {
            const uint32_t a = (SVH_DIAG_AB == 1 || FL) ? 0u : j % NS, b2 = FL ? 0u : j % kNE;
            const float4 h = make_float4(hq[4 * a], hq[4 * a + 1], hq[4 * a + 2], hq[4 * a + 3]);
            const float xs = SX ? xq[(SVH_DIAG_AB == 1 || FL) ? 0u : j % (2 * kAG)] : 0.0f;
            const f2 e = DM == 2 ? (f2){eq[4 * b2], eq[4 * b2 + 1]} : (f2){eq[2 * b2], eq[2 * b2 + 1]};
            // at even steps, together: the constants of steps j + kPS and j + kPS + 1 (the next block's
            // past kDK - 1), then the ring pairs of steps j + kPE and j + kPE + 1, then, every kAG
            // steps, the ring addresses of steps j + 2 kAG .. (into the slot of the group whose last
            // pairs were just issued) and the X_SF of steps j + kAG ...  Whatever a read needs is
            // older than the pairs the steps last waited for, so the only wait of two steps is the
            // one for this step's and the next's pairs, with the reads issued since left in flight
            // (four here and one group read, this step's or the one two steps back).  The compiler
            // places its own counted waits where this one does not suffice: the count is a matter
            // of speed only.
            if (RP == 0 && j % 2 == 0) {
                if (SVH_DIAG_AB != 1 && !FL) {
                    sread(kb, j + kPS, (j + kPS) % kNS);
                    sread(kb, j + kPS + 1, (j + kPS + 1) % kNS);
                }
                if (SVH_DIAG_AB != 2 && !FL) {
                    eread(j + kPE);
                    eread(j + kPE + 1);
                }
                if (SVH_DIAG_AB != 1 && !FL && j % kAG == 0) {
                    gread(aq, adr, kb, j + 2 * kAG);
                    if (SX) gread(xq, xsf, kb, j + kAG);
                }
                if (SVH_DIAG_AB == 0 && !FL) {
                    // lgkmcnt(5 or 6) alone (PATHS: and the two ring writes since the pairs' reads;
                    // DM = 2: the pairs of two steps are four reads; QD: two again, one quad per step)
                    __builtin_amdgcn_s_waitcnt(0xC07F | (((SX ? 6 : 5) + (PATHS ? 2 : 0) + (DM == 2 && !QD ? 2 : 0)) << 8));
                    __builtin_amdgcn_sched_barrier(0);                         // ahead of both steps' uses
                }
            }
            // The quad ring's read placement (RP = 1): the same reads as above with the quads' two
            // address adds ahead of them in every body (the order above leaves one between the reads
            // in the bodies that read an address group), so that the two constants, the two quads
            // and the group read(s) issue in one run, and with the constants two steps ahead like the
            // quads; everything fenced where it stands.  The wait's count: a body consumes the reads
            // of the body before, LDS reads return in order, and behind that body's last read stand
            // this body's four and, every other body, its group read (two with SX): lgkmcnt(4) or
            // lgkmcnt(5 or 6).  The quads' distance is kPE as above: ring timing as it was.
            if constexpr (RP == 1) {
                if (j % 2 == 0) {
                    uint32_t qa[2];
#pragma unroll
                    for (uint32_t i = 0; i < 2; ++i) {
                        const float roff = aq[(j + kPE + i) % (2 * kAG)];
                        qa[i] = __builtin_bit_cast(uint32_t, roff) + lane * 16u;
                        asm volatile("" : "+v"(qa[i]));
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    sread(kb, j + PS, (j + PS) % NS);
                    sread(kb, j + PS + 1, (j + PS + 1) % NS);
#pragma unroll
                    for (uint32_t i = 0; i < 2; ++i) {
                        const f4 e4 = lds_ld4(qa[i]);
                        eq[4 * ((j + kPE + i) % kNE)] = e4.x;
                        eq[4 * ((j + kPE + i) % kNE) + 1] = e4.y;
                        eq[4 * ((j + kPE + i) % kNE) + 2] = e4.z;
                        eq[4 * ((j + kPE + i) % kNE) + 3] = e4.w;
                    }
                    if (j % kAG == 0) {
                        gread(aq, adr, kb, j + 2 * kAG);
                        if (SX) gread(xq, xsf, kb, j + kAG);
                        __builtin_amdgcn_s_waitcnt(0xC07F | ((SX ? 6 : 5) << 8));
                    } else {
                        __builtin_amdgcn_s_waitcnt(0xC07F | (4 << 8));
                    }
                    __builtin_amdgcn_sched_barrier(0);  // ahead of both steps' uses
                }
            }
            if constexpr (DM == 2) step2(h, xs, e, (f2){eq[4 * b2 + 2], eq[4 * b2 + 3]});
            else step(h, xs, e, j % kFS);
            if (j % 2 == 1) __builtin_amdgcn_sched_barrier(0);  // keep the reads where they are issued
            if constexpr (PATHS) {
                if (j % kFS == kFS - 1 && (SVH_DIAG_PAB != 4 || j == kDK - 1)) {
                    exec_collect(alive);
                    if (SVH_DIAG_PAB == 4) {
                        fold(kb * kDK + 1 + j - (kFS - 1), kFS);
                    } else {  // the group before this one, then this one's reads; the block's last at once
                        if (j >= kFS) fold_min(kb * kDK + 1 + j - (2 * kFS - 1), kFS);
                        fold_read();
                        if (j == kDK - 1) fold_min(kb * kDK + 1 + j - (kFS - 1), kFS);
                    }
                    if (j == 31) keep32();
                    if (j == kDK - 1) block_records(kb, kDK);
                    __builtin_amdgcn_sched_barrier(0);  // the next steps' first check stays below
                }
            }
        }
        if constexpr (!PATHS) exec_collect(alive);
    };
    // the row's last, partial block: plain steps
    auto tail = [&](uint32_t kb, uint32_t rem) {
        const uint32_t e0 = LD ? (w * NB + kb % NB) * kDK : (w * 2 + (kb & 1u)) * kDK;
        if constexpr (PATHS) {  // groups of kFS steps, each with its collect and fold
            for (uint32_t g0 = 0; g0 < rem; g0 += kFS) {
                const uint32_t n = rem - g0 < kFS ? rem - g0 : kFS;
                __builtin_amdgcn_sched_barrier(0);
                for (uint32_t j = g0; j < g0 + n; ++j) {
                    const float4 h = *reinterpret_cast<const float4*>(strm + (e0 + j) * kDE);
                    const float roff = adr[e0 + j];
                    step(h, SX ? xsf[e0 + j] : 0.0f, lds_ld2(__builtin_bit_cast(uint32_t, roff) + lane * 8u), j - g0);
                }
                exec_collect(alive);
                fold(kb * kDK + 1 + g0, n);
                if (g0 + n == 32 && rem > 32) keep32();
            }
            block_records(kb, rem);
            return;
        }
        __builtin_amdgcn_sched_barrier(0);
        for (uint32_t j = 0; j < rem; ++j) {
            const float4 h = *reinterpret_cast<const float4*>(strm + (e0 + j) * kDE);
            const float roff = adr[e0 + j];
            if constexpr (QD) {
                const f4 e = lds_ld4(__builtin_bit_cast(uint32_t, roff) + lane * 16u);
                step2(h, SX ? xsf[e0 + j] : 0.0f, (f2){e.x, e.y}, (f2){e.z, e.w});
            } else if constexpr (DM == 2) {
                const uint32_t a = __builtin_bit_cast(uint32_t, roff) + lane * 4u;
                step2(h, SX ? xsf[e0 + j] : 0.0f, (f2){lds_ld1(a), lds_ld1(a + 256u)},
                      (f2){lds_ld1(a + kDRS2 * 4u), lds_ld1(a + kDRS2 * 4u + 256u)});
            } else {
                step(h, SX ? xsf[e0 + j] : 0.0f, lds_ld2(__builtin_bit_cast(uint32_t, roff) + lane * 8u));
            }
        }
        exec_collect(alive);  // right behind the loop's scalar branch: no other branch sees a partial EXEC
    };

    if constexpr (LD) {
        if (ldr) {
            // the loader wave: during block k the refill of group k + 4 (loaded one block earlier; into
            // the slots of group k - 1, last read in block k - 1), the loads of group k + 5, the streams
            // of block k + 2 (into the buffer of block k - 1) and the symbols of block k + 3; its LDS
            // writes are complete (lgkmcnt(0)) when it arrives at the block's barrier
            // Quad ring timing (QD): group k + 4 is issued during block k and has landed in LDS when this
            // wave's vmcnt(0) below completes, ahead of barrier k (the one that ends block k).  Its first
            // reader is a step wave's prefetch at the end of block k + 2 (block kb reads columns
            // 64 kb + 1 .. 64 kb + 130: groups kb .. kb + 2), behind barriers k and k + 1, which that wave
            // has passed: an LDS-DMA write is ordered for another wave's read by the issuer's vmcnt and a
            // barrier, and here there are two.  The slots it lands in are those of group k - 1 (and, every
            // fifth block, the mirror, last read in block k - 2), last read in block k - 1 by reads whose
            // values the steps of that block used, so they had returned before barrier k - 1, which this
            // wave passed before issuing.  (The wait could move behind barrier k, ahead of barrier k + 1,
            // by the same argument; the loader wave has nothing to do in that time, so it stays here.)
            for (uint32_t k = 0; k < nbmax; ++k) {
                if constexpr (QD) {
                    sbuildl(k + 2);
                    symloadl(k + 3);
                    qfill(k + 4, 0, 1);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                } else if (!flr) {
                    sbuildl(k + 2);
                    symloadl(k + 3);
                    lwritel(k + 4);
                    gloadl(k + 5);
                }
                lds_barrier();
            }
            return;  // (ends here: see the note on S_BARRIER above the kernel)
        }
    }
    for (uint32_t k = 0; k < nbmax; ++k) {
        const uint32_t rem = k < nb ? nst - k * kDK : 0u;
        const bool full = k < nb && rem >= kDK;
        // (issuing this work between the block's steps instead measured the same: 0.1940 against
        // 0.1934 ms; the per-block cost is the barrier and its LDS drain, profiles/r06_diag/)
        if constexpr (!LD) blockwork(k);
        if (k < nb) {
            if (full) block(k);
            else tail(k, rem);
        }
        if (SVH_DIAG_AB != 3) lds_barrier();
    }

    F = FC.x;
    c = FC.y;
    xv = DM == 2 ? X2.x : XP.x;
    xv2 = X2.y;

    // ---- scores of the light positions and this wave's partials
#if SVH_DIAG_AB == 5  // diagnostics: the scores only (every wave leaves here)
    if (real && m.lrow[(rg * 64 + lane + nst) % NP] != kNoRow)
        g_st_score(b.scores + (size_t)q * m.n + m.lrow[(rg * 64 + lane + nst) % NP], xv);
    return;
#endif
    uint32_t last = 0;
    if (real) {
        float* out = b.scores + (size_t)q * m.n;
        const uint32_t pe = (rg * RW + lane + nst) % NP;
        const uint32_t r = m.lrow[pe];
        float bv = kInf;
        uint32_t bk = kNoRow;
        if (r != kNoRow) {
            g_st_score(out + r, xv);  // the row's re-run may come from another XCD
            bv = xv;
            bk = r;
        }
        if constexpr (DM == 2) {  // the second diagonal, 64 positions on
            const uint32_t r2 = m.lrow[pe + 64 >= NP ? pe + 64 - NP : pe + 64];
            if (r2 != kNoRow) {
                g_st_score(out + r2, xv2);
                lex_min(bv, bk, xv2, r2);
            }
        }
        wave_lexmin63(bv, bk);
        const float cmin = wave_min63(c);
        const bool any_viol = alive != ~0ull;
        if (lane == 63 && !flr) {
            uint64_t* part = x.part + ((size_t)q * x.G + rg) * 2;
            g_st64(part, ((uint64_t)(any_viol ? 1u : 0u) << 32) | __builtin_bit_cast(uint32_t, cmin));
            g_st64(part + 1, lex_key(bv, bk));
#if SVH_DIAG_AB == 7  // diagnostics: no arrival count (the last range combines, unordered)
            last = rg == NR - 1 ? 1u : 0u;
#else
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const uint32_t d = __hip_atomic_fetch_add(x.done + (size_t)q * SVH_DIAG_DONE_STRIDE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            last = d == NR - 1 ? 1u : 0u;
#endif
#if SVH_DIAG_AB == 8  // diagnostics: the arrival count, no combine
            last = 0;
#endif
        }
        last = readlane_u(last, 63);
    }
    if (last) {  // this wave combines sequence q: lanes read the ranges' partials
        float C = kInf, bv2 = kInf;
        uint32_t bk2 = kNoRow, vi = 0;
        for (uint32_t u = lane; u < NR; u += 64) {
            const uint64_t* pu = x.part + ((size_t)q * x.G + u) * 2;
            const uint64_t a = g_ld64(pu), k2 = g_ld64(pu + 1);
            C = fminf(C, __builtin_bit_cast(float, (uint32_t)a));
            vi |= (uint32_t)(a >> 32);
            if (k2 != ~0ull) lex_min(bv2, bk2, lex_key_value(k2), lex_key_index(k2));
        }
        C = wave_min63(C);
        wave_lexmin63(bv2, bk2);
        const bool any = __builtin_amdgcn_ballot_w64(vi != 0) != 0;
        if (lane == 63) {
            float* out = b.scores + (size_t)q * m.n;
            if (m.rowF >= 0) {
                out[m.rowF] = F;
                lex_min(bv2, bk2, F, (uint32_t)m.rowF);
            }
            if (m.rowS >= 0) {
                out[m.rowS] = C;
                lex_min(bv2, bk2, C, (uint32_t)m.rowS);
            }
            if (b.best) b.best[q] = bk2 == kNoRow ? -1 : (int64_t)bk2;
            x.viol[q] = any ? 1u : 0u;
            __hip_atomic_store(x.done + (size_t)q * SVH_DIAG_DONE_STRIDE, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (any && !PATHS) rrow[w] = q;
        }
    }
    // rows whose speculation failed: re-run exactly by this workgroup (pipe_rerun_row, the latency
    // plan's serial recurrence with F's light term restored) -- no second launch on the common path
    if constexpr (PATHS) return;  // (the host's chain fallback re-runs them with their path records)
    __syncthreads();
    uint32_t rq[W];  // read before any re-run: its scores overwrite this part of the LDS
#pragma unroll
    for (int u = 0; u < W; ++u) rq[u] = rrow[u];
#pragma unroll
    for (int u = 0; u < W; ++u) {
        if (rq[u] != kNoRow) {
            __syncthreads();
            pipe_rerun_row<2, W, SX>(m, b, rq[u], lds);
        }
    }
