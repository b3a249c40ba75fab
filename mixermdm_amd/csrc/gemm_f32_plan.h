// The dispatch rule of the exact-fp32 linear layer (gemm_f32.hip) as a pure host function: which kernel(s) a call launches, on which rows.
// Plain C++17, no HIP headers, no globals: gemm_f32.hip walks the plan through its launcher table, tests/test_gemm_f32_plan_cpu.py compiles
// this header alone and holds it to its Python statement (tests/gemm_f32_cases.py) on the CPU.  The kernel list, the names
// mmdm_last_gemm_kernel() reports and the rule each exist here and nowhere else.
#pragma once
#include <stdio.h>
#include "../../include/mmdm.h"

namespace gemm_f32_plan {

// Every kernel form a plan can name, with its note.  A two-form kernel lists its second form (16-byte epilogue "vepi" / late residual)
// directly behind the first: form().  gemm_f32 stands for its five load forms, a gemm_glds / gemm_pipe entry also for its stamping twin.
#define GEMM_F32_KERNELS(X)                                                                                      \
    X(F32, "gemm_f32<22,22,16>")                                                                                 \
    X(GLDS_2221, "gemm_glds<22,21,16,2,scalar>") X(GLDS_2221_V, "gemm_glds<22,21,16,2,vepi>")                    \
    X(GLDS_2222, "gemm_glds<22,22,16,2,scalar>") X(GLDS_2222_V, "gemm_glds<22,22,16,2,vepi>")                    \
    X(PIPE_2121, "gemm_pipe<21,21,16,4,scalar>") X(PIPE_2121_V, "gemm_pipe<21,21,16,4,vepi>")                    \
    X(PIPE_2221, "gemm_pipe<22,21,16,4,scalar>") X(PIPE_2221_V, "gemm_pipe<22,21,16,4,vepi>")                    \
    X(PIPE_2222, "gemm_pipe<22,22,16,5,scalar>") X(PIPE_2222_V, "gemm_pipe<22,22,16,5,vepi>")                    \
    X(S16_13, "gemm_s16<1,3,plain>") X(S16_13_L, "gemm_s16<1,3,late>")                                           \
    X(S16_23, "gemm_s16<2,3,plain>") X(S16_23_L, "gemm_s16<2,3,late>")                                           \
    X(S16_14, "gemm_s16<1,4,plain>") X(S16_14_L, "gemm_s16<1,4,late>")                                           \
    X(S16_24, "gemm_s16<2,4,plain>") X(S16_24_L, "gemm_s16<2,4,late>")                                           \
    X(MIX, "gemm_mix<scalar,%d+%d>") X(MIX_V, "gemm_mix<vepi,%d+%d>")

enum Kernel {
#define X(id, name) id,
    GEMM_F32_KERNELS(X)
#undef X
    KERNEL_COUNT
};
inline Kernel form(Kernel first, bool second) { return Kernel(first + (second ? 1 : 0)); }

// One call.  The alignment facts are about pointers and leading dimensions only: a_vec / w_vec: A / W 16-byte aligned with ld % 4 == 0;
// c_al: the same of C; bias_al: bias null or 16-byte aligned; extra_al: `extra` 16-byte aligned with ld_extra % 4 == 0 (read for resid / pe only).
// cfg: the gemm_cfg switch; tail: the row-split rule in force (the forced gemm_tail, else the thread's); s16: the gemm_s16 switch.
struct Call {
    int M, N, K, Kw, epilogue;
    bool a_vec, w_vec, c_al, bias_al, extra_al;
    int cfg, tail, s16;
};
// A launch computes rows [row0, row0 + rows) of the call; M1 (MIX only): its first M1 rows run on the 64 x 64 tiles, the others on the 16 x 16 chains.
struct Launch { Kernel kernel; int row0, rows, M1; };
struct Plan { int n; Launch l[2]; };      // n = 1, or 2: the row split, main launch first

inline long cdiv(long a, long b) { return (a + b - 1) / b; }
inline bool reads_extra(const Call& c) { return c.epilogue == MMDM_EPI_BIAS_RESID || c.epilogue == MMDM_EPI_BIAS_PE; }
// 16-byte operand loads of A / W rows (Kw >= K: readable columns of W)
inline bool a_vec4(const Call& c) { return c.a_vec && c.K % 4 == 0; }
inline bool w_vec4(const Call& c) { return c.w_vec && c.Kw % 4 == 0; }
// the LDS-DMA kernels (gemm_glds, gemm_pipe): whole K steps of 16 through 16-byte pieces
inline bool glds_ok(const Call& c) { return a_vec4(c) && w_vec4(c) && c.K % 16 == 0 && c.Kw == c.K; }
// the 16-byte epilogue: bias / residual / PE quads in, result quads out
inline bool vepi_ok(const Call& c) { return c.N % 4 == 0 && c.c_al && c.bias_al && (!reads_extra(c) || c.extra_al); }
// gemm_s16: those accesses in every epilogue, K steps of 32
inline bool s16_ok(const Call& c) { return vepi_ok(c) && c.K % 32 == 0 && c.Kw == c.K; }
// shapes whose best pipelined tile is 128 x 64 with 4 stages (three workgroups per CU), not 128 x 128 with 5 (two)
inline bool narrow_tile(const Call& c) { return c.N <= 512 || c.K <= 512 || c.N == 2048; }

inline Plan one(Kernel k, const Call& c, int M1 = 0) { return Plan{1, {{k, 0, c.M, M1}, {k, 0, 0, 0}}}; }

// The automatic rule for operands the LDS-DMA kernels take (glds_ok).  The 16-byte epilogue pays where the accumulators' addend is read
// from memory and is neutral-to-negative otherwise, so only the residual / PE epilogues take it.  Every pipelined form, gemm_s16 and
// gemm_mix accumulate an output element in the same order: the choice of tile never changes a bit.
inline Plan automatic(const Call& c) {
    const int M = c.M, N = c.N, K = c.K;
    const bool vepi = reads_extra(c) && vepi_ok(c);
    if (K < 96)          // too short for the pipelined loop's prologue: the 2-stage kernels
        return one(form(cdiv(M, 128) * cdiv(N, 128) < 1000 ? GLDS_2221 : GLDS_2222, vepi), c);
    const bool narrow = narrow_tile(c);
    if (c.tail && c.epilogue != MMDM_EPI_BIAS_PE) {
        // Row split for callers that run ONE stream of kernels (the two-stream step's other stream already fills a tail): the fractional last
        // round of 512 (128x128, two per CU) or 768 (128x64, three per CU) resident tiles costs a whole tile lifetime on a partly empty chip.
        // Rows [0, M1) -- the whole row tiles of the complete rounds -- go to the large tile, the others to a tile of half / a quarter of the
        // area (configs[1], M = 12 544: 15.35 -> 14.45 ms/step).  Not for the PE epilogue: the row index would restart in the remainder.
        const long slots = narrow ? 768 : 512, nt = cdiv(N, narrow ? 64 : 128), mt = cdiv(M, 128);
        const long tiles = mt * nt, full = tiles / slots, rem = tiles - full * slots, mt1 = full * slots / nt;
        if (mt * cdiv(N, 64) >= 512 && full >= 1 && mt1 >= 1 && mt1 < mt && rem * 10 <= slots * c.tail) {
            const int M1 = (int)mt1 * 128;
            // remainder: the largest tile that still gives every CU a workgroup
            const bool half = !narrow && cdiv(M - M1, 128) * cdiv(N, 64) >= 256;
            return Plan{2, {{form(narrow ? PIPE_2221 : PIPE_2222, vepi), 0, M1, 0}, {form(half ? PIPE_2221 : PIPE_2121, vepi), M1, M - M1, 0}}};
        }
    }
    const bool late = reads_extra(c);
    if (c.s16 > 0 && s16_ok(c)) return one(form(c.s16 == 13 ? S16_13 : c.s16 == 14 ? S16_14 : c.s16 == 24 ? S16_24 : S16_23, late), c);
    // Launches whose 64 x 64 grid leaves half of the CUs idle (configs[0]'s M = 240 against N <= 2048, conditioning / time-embedding rows):
    // quarter-length chains on 16 x 16 blocks, four times the workgroups.  Not the weight-streaming projections (M <= 64 against N >= 4096).
    const bool streams64 = M <= 64 && N >= 4096;
    if (c.s16 < 0 && cdiv(M, 64) * cdiv(N, 64) <= 128 && !streams64 && s16_ok(c)) return one(form(S16_14, late), c);
    const long t64 = cdiv(M, 128) * cdiv(N, 64);
    // 64 x 64 tiles with a fractional last round (the reference's B = 1 call, M = 1196): the rows of the whole rounds of 256 on those tiles,
    // the rest as quarter-length chains beside them, in one launch.  The remainder tiles cost about twice their matrix-pipe time, so only for
    // one or two whole rounds and a remainder no larger than the main part (tools/gemm_s16_bench.py: N = 1024 37.6 -> 30.1 us, N = 3072 79.8 -> 82.7).
    if (t64 < 512 && c.s16 < 0 && c.epilogue != MMDM_EPI_BIAS_PE && s16_ok(c)) {
        const long nt64 = cdiv(N, 64), tiles = cdiv(M, 64) * nt64, rounds = tiles / 256, mt1 = rounds * 256 / nt64;
        const long rem_wgs = mt1 * 64 < M ? cdiv(M - mt1 * 64, 32) * cdiv(N, 32) : 0;
        if (rounds >= 1 && rounds <= 2 && mt1 >= 1 && rem_wgs > 0 && rem_wgs <= mt1 * nt64 && tiles % 256 != 0)
            return one(form(MIX, c.epilogue == MMDM_EPI_BIAS_RESID), c, (int)mt1 * 64);
    }
    // Few tiles (small batches): 64 x 64 tiles so that every CU has work.  Skinny M against a wide weight matrix (the packed AdaLN projections,
    // 134 / 201 MB of weights read once per step) streams weights: M <= 64, N = 49 152 takes 158 us on 128 x 128 tiles, 79 us on 64 x 64 (more
    // bytes in flight); 128 x 64 for 64 < M <= 256: 134 -> 110 us (M = 128).
    if (t64 < 512 || streams64) return one(form(PIPE_2121, vepi), c);
    // Tile / stage choice measured at M = 19 200 (tools/gemm_bench.py, TFLOP/s): N = 3072, K = 1024 (QKV): 128x128, 5 stages 128; N = 1024,
    // K = 1024 / 2048: 128x128, 5 stages 124 / 128; N = 2048, K = 1024 (FFN up, K|V): 128x64, 4 stages 119-122; mixer (N or K <= 512): 107-121
    if ((M <= 256 && N >= 4096) || narrow) return one(form(PIPE_2221, vepi), c);
    return one(form(PIPE_2222, vepi), c);
}

// gemm_cfg: -1 the automatic rule; 11 / 17 the 2-stage kernels 128 x 128 / 128 x 64; 34 / 36 / 41 the pipelined 128 x 128 (5 stages) /
// 128 x 64 / 64 x 64 (4 stages), each from the K that fills its stages; every other value, and every call whose operands the forced kernel
// does not take, the register-staged fallback.
inline Plan plan(const Call& c) {
    if (glds_ok(c)) {
        const bool vepi = reads_extra(c) && vepi_ok(c);
        switch (c.cfg) {
            case -1: return automatic(c);
            case 11: return one(form(GLDS_2222, vepi), c);
            case 17: return one(form(GLDS_2221, vepi), c);
            case 34: if (c.K >= 80) return one(form(PIPE_2222, vepi), c); break;
            case 36: if (c.K >= 64) return one(form(PIPE_2221, vepi), c); break;
            case 41: if (c.K >= 64) return one(form(PIPE_2121, vepi), c); break;
            default: break;
        }
    }
    return one(F32, c);
}

// the note of a launch of a call with N columns: mmdm_last_gemm_kernel() joins a plan's notes with "+"
inline void kernel_name(const Launch& l, int N, char* out, size_t size) {
    static const char* const names[KERNEL_COUNT] = {
#define X(id, name) name,
        GEMM_F32_KERNELS(X)
#undef X
    };
    // gemm_mix<form,a+b>: a workgroups of 64 x 64 + b of 32 x 32 (the other names hold no conversion)
    snprintf(out, size, names[l.kernel], (int)(l.M1 / 64 * cdiv(N, 64)), (int)(cdiv(l.rows - l.M1, 32) * cdiv(N, 32)));
}

}  // namespace gemm_f32_plan
