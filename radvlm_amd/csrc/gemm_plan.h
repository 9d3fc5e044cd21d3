// The launch shape of one GEMM call, decided on the host: plain C++ without HIP or global state, so the decision can be checked (and
// run under host sanitizers) without a device.  gemm_bf16.hip keeps the one GemmConfig of the process and launches what gemm_plan
// returns; rv_gemm_plan reports it.  DESIGN.md section 4b lists every shape, what selects it and the test that pins it.
#pragma once
#include <stdint.h>

constexpr int PLAN_TILE128 = 128, PLAN_TILE256 = 256, PLAN_BK = 64;   // the tiles of the two kernels and the K-tile (asserted in gemm_bf16.hip)

// Process-wide launch configuration.  None of it depends on the arguments of a call; results never depend on it (only which launch
// shape computes them).
struct GemmConfig {
    int cus = 0;            // compute units the tile-round heuristics plan for (rv_gemm_set_cu_budget: the device's units minus those
                            // reserved for concurrently running collectives, at least 8); 0 = not yet established
    int force_kernel = 0;   // 0 auto, 1 = 128x128 kernel, 2 = 256x256 kernel (RV_GEMM_KERNEL or rv_gemm_select_kernel)
    int tail_split = 1;     // rv_gemm_select_kernel(20 / 21): tail split off / on (A/B measurement)
    int flat = 0;           // rv_gemm_select_kernel(30 / 31): flat staging (buffer-addressed off) / buffer-addressed (A/B measurement)
    int persist = 1;        // rv_gemm_select_kernel(40 / 41): persistent tile-walking blocks off / on.  OFF when collectives share the GPU
                            // (the engine does that for world size > 1): a persistent block that cannot start because an RCCL kernel holds
                            // its CU delays its whole share of the tiles (up to 2x for the launch); one-tile blocks only lose part of a round
};
// GEMM_PLAIN: rv_gemm_bf16_ex.  GEMM_DROPOUT: the dropout epilogue -- no K-split (the reduce kernels do not carry the mask), always the
// 256x256 kernel.  GEMM_FUSED: a fused epilogue (RoPE, SwiGLU) -- no K-split, no second pair; the kernel follows the round-cost rule or the
// forced kernel WHATEVER the layouts, and "not the 256x256 kernel" means the entry point runs the unfused sequence.
enum GemmKind { GEMM_PLAIN = 0, GEMM_DROPOUT = 1, GEMM_FUSED = 2 };
struct GemmRequest {        // K2 = 0: no second operand pair; workspace_bytes = 0: no workspace
    int M, N, K, trans_a, trans_b;
    int64_t lda, ldb;
    int K2;
    int64_t lda2, ldb2, workspace_bytes;
    int kind;
};
struct GemmPlan {
    int use256;             // 256x256 kernel (else the 128x128 one: plain NT whole tiles only)
    int mode;               // MODE of gemm_kernel_256: 0 whole tiles, 1 second operand pair, 2 split-K, 3 tail split
    int splits;             // K-slices per tile (MODE 2) / per tail tile (MODE 3); 1 otherwise
    int n_full;             // MODE 3: tiles computed whole; 0 otherwise
    int grid, pgrid;        // blocks of the GEMM kernel; GemmParams::pgrid of that launch
    int buf;                // buffer-addressed staging
    int tiles_m, tiles_n;   // output tiles of the chosen kernel
    unsigned bytesA, bytesB, bytesA2, bytesB2;   // buf: the operand extents of the buffer resources (the second pair's in MODE 1)
};

// The ABI's preconditions on sizes and leading dimensions: 16-byte rows and row starts for every operand in its layout.
inline bool gemm_args_ok(const GemmRequest& q) {
    if (q.M <= 0 || q.N <= 0 || q.K <= 0 || q.K2 < 0 || q.workspace_bytes < 0 || q.kind < GEMM_PLAIN || q.kind > GEMM_FUSED) return false;
    if ((q.lda & 7) || (q.ldb & 7)) return false;
    if ((!q.trans_a && (q.K & 7)) || (q.trans_a && (q.M & 7)) || (!q.trans_b && (q.K & 7)) || (q.trans_b && (q.N & 7))) return false;
    return !(q.K2 > 0 && ((q.lda2 & 7) || (q.ldb2 & 7) || (!q.trans_a && (q.K2 & 7)) || (!q.trans_b && (q.K2 & 7))));
}
// Tile-shape choice, the round-cost rule: whole rounds of `cus` blocks (256^2 tiles, 1 block/CU) against double-rounds of 2 x cus blocks
// (128^2 tiles, 2 blocks/CU, ~15 % less efficient per flop but finer grained); measured crossover on MI355X (tools/ab_kernel12.py):
// 292 / 352 tiles -> 128^2 wins by 8-27 %, >= 876 tiles -> 256^2 wins by 3-7 %.
inline bool gemm_prefers_256(int64_t tiles256, int64_t tiles128, const GemmConfig& c) {
    if (c.force_kernel) return c.force_kernel == 2;
    return 4.0 * (double)((tiles256 + c.cus - 1) / c.cus) <= 2.0 * 1.15 * (double)((tiles128 + 2 * c.cus - 1) / (2 * c.cus));
}
// Extents of one operand pair for the buffer-addressed kernels; false when it does not qualify (K tail inside a row, >= 2 GiB operand).
// A K tail is a resource boundary only for contraction-major operands (whole rows past the end read as zero); inside the rows of a
// row-major operand it is not -- e.g. the weight gradients of a 14998-token batch (both operands contraction-major) qualify.
inline bool gemm_operand_extents(int M, int N, int K, int trans_a, int trans_b, int64_t lda, int64_t ldb, unsigned& bytes_a, unsigned& bytes_b) {
    const int64_t lim = INT64_C(1) << 31;
    if (((K % PLAN_BK) && !(trans_a && trans_b)) || lda < 0 || ldb < 0 || lda >= lim || ldb >= lim) return false;    // ld < 2^31: the products stay inside int64
    const int64_t ea = (int64_t)(trans_a ? K : M) * lda * 2, eb = (int64_t)(trans_b ? K : N) * ldb * 2;
    if (ea >= lim || eb >= lim) return false;
    bytes_a = (unsigned)ea; bytes_b = (unsigned)eb;
    return true;
}

// Pure: c.cus > 0 and gemm_args_ok(q) are the caller's to establish.
inline GemmPlan gemm_plan(const GemmRequest& q, const GemmConfig& c) {
    const int cus = c.cus;                  // 256 on an idle MI355X; fewer when collectives are planned to run beside the GEMMs
    GemmPlan pl = {};
    pl.mode = q.kind != GEMM_FUSED && q.K2 > 0 ? 1 : 0;
    pl.splits = 1;
    pl.tiles_m = (q.M + PLAN_TILE256 - 1) / PLAN_TILE256; pl.tiles_n = (q.N + PLAN_TILE256 - 1) / PLAN_TILE256;
    const int64_t tiles256 = (int64_t)pl.tiles_m * pl.tiles_n, ws_bytes = q.kind == GEMM_PLAIN && pl.mode == 0 ? q.workspace_bytes : 0;
    const int nt = (q.K + PLAN_BK - 1) / PLAN_BK;
    // split-K: few output tiles but a long contraction (LoRA / bias-like gradients): spread K over the idle CUs
    if (ws_bytes > 0 && tiles256 <= cus / 4 && nt >= 16) {
        int sp = (int)(cus / tiles256);
        if (sp > nt / 4) sp = nt / 4;
        if (sp > 32) sp = 32;
        if (sp >= 2 && (int64_t)sp * q.M * q.N * 4 <= ws_bytes) { pl.mode = 2; pl.splits = sp; }
    }
    // tail split: when the last round of `cus` blocks is at most half full, its tiles are cut into 2-4 K-slices so that the
    // round costs 1/2 - 1/4 of a full one (e.g. 1408 tiles on 256 CUs: 6 rounds -> 5.5)
    if (ws_bytes > 0 && pl.mode == 0 && c.tail_split && tiles256 > cus) {
        const int rem = (int)(tiles256 % cus), sp = rem && cus / rem < 4 ? cus / rem : 4;
        if (rem > 0 && rem <= cus / 2 && nt >= 32 && (int64_t)rem * sp * PLAN_TILE256 * PLAN_TILE256 * 4 <= ws_bytes) {
            pl.mode = 3; pl.splits = sp; pl.n_full = (int)(tiles256 - rem);
        }
    }
    // the 128x128 kernel only exists for the plain NT form; a fused epilogue only in the 256x256 kernel
    const int tm128 = (q.M + PLAN_TILE128 - 1) / PLAN_TILE128, tn128 = (q.N + PLAN_TILE128 - 1) / PLAN_TILE128;
    const bool by_cost = q.kind == GEMM_FUSED || (q.kind == GEMM_PLAIN && !q.trans_a && !q.trans_b && !pl.mode);
    pl.use256 = !by_cost || gemm_prefers_256(tiles256, (int64_t)tm128 * tn128, c);
    if (!pl.use256) { pl.tiles_m = tm128; pl.tiles_n = tn128; pl.grid = pl.pgrid = tm128 * tn128; return pl; }
    // staging: buffer-addressed when every operand the mode reads qualifies (MODE 1: both pairs)
    pl.buf = !c.flat && gemm_operand_extents(q.M, q.N, q.K, q.trans_a, q.trans_b, q.lda, q.ldb, pl.bytesA, pl.bytesB) &&
             (pl.mode != 1 || gemm_operand_extents(q.M, q.N, q.K2, q.trans_a, q.trans_b, q.lda2, q.ldb2, pl.bytesA2, pl.bytesB2));
    if (!pl.buf) pl.bytesA = pl.bytesB = pl.bytesA2 = pl.bytesB2 = 0;
    const int nwg = (int)tiles256;
    pl.pgrid = pl.mode == 2 ? nwg * pl.splits : (pl.mode == 3 ? pl.n_full : nwg);
    // persistent form: one block per CU walks the whole tiles (MODE 3: + the K-slice blocks of the tail tiles behind them)
    if (c.persist && pl.buf && pl.mode != 2 && pl.pgrid > cus) pl.pgrid = cus;
    pl.grid = pl.pgrid + (pl.mode == 3 ? (nwg - pl.n_full) * pl.splits : 0);
    return pl;
}
