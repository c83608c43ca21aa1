// The entry lookup of the model sets' kernels (diag.hip diag_set_kernel, diag_set_paths_kernel),
// included at the top of the kernel: in scope the arguments `e`, `first`, `ne` and the constant PATHS;
// it leaves `m`, `b`, `x` (the entry's triple) and `bx` (the workgroup's index within that entry's own
// grid) for diag_body.h.  Text for the body's reason: the scores kernels stay instruction for
// instruction what they were.
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
    if constexpr (PATHS)
        in_global(ent.b.cmask, ent.b.cmask_off, ent.b.ckpt, ent.b.ckpt_off, ent.b.prec, ent.b.prec_off, ent.b.fck, ent.b.fck_off,
                  ent.b.hrec, ent.b.hrec_off);
    const PipeModel& m = ent.m;
    const FusedBatch& b = ent.b;
    const PipeScratch& x = ent.x;
    const uint32_t bx = gbx - f0;
