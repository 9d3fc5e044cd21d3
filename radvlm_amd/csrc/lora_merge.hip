// LoRA merge for gfx950: W[N,K] <- bf16(float(W) + scale * B[N,r] A[r,K]), in place (peft merge_and_unload, W += (alpha / r) B A).
// One read and one write of W is the whole HBM traffic; A and B (r <= 256) are read from L2.  The rank-r product runs on
// v_mfma_f32_16x16x32_bf16 with r zero-padded to a multiple of 32 (a VALU dot product of r = 64 would make the kernel compute-bound at
// the 13B size).  Every element's sum is the MFMA's fixed k order over j = 0 .. rpad - 1, added to W once and rounded once: the bits do
// not depend on the grid, on N or on where W sits in a fused store.
#include "common.h"
#include "radvlm_hip.h"

#include <stdlib.h>

namespace {

constexpr int LM_COLS = 64;             // W columns per block: four 16-column MFMA tiles
constexpr int LM_ROWS = 64;             // W rows per row tile: one 16-row MFMA tile per wave
constexpr int LM_RED_LD = LM_COLS + 4;  // fp32 product tile row stride (floats)
constexpr int LM_BLOCKS = 2048;         // target grid size (row tiles per block grow beyond it)

// Block: W columns [k0, k0 + 64) x row tiles [rt0, rt1) of 64 rows.  The A strip A[:, k0:k0+64] is staged once, transposed (at[col][j]),
// so each lane's MFMA B operand (A[j = 8(l>>4) .. +7][col l&15]) is one 16-byte LDS read.  Per row tile: wave w computes rows 16w .. +15
// (MFMA A operand = B rows, lane l: row l&15, j = 8(l>>4) .. +7), the 64 x 64 fp32 product goes through LDS, and every thread then
// adds it to 2 x 8 contiguous W elements loaded (16 bytes each) before the MFMAs.
template <bool NT>
__global__ __launch_bounds__(256) void lora_merge_kernel(bf16* __restrict__ W, long ldw, const bf16* __restrict__ B, long ldb,
                                                         const bf16* __restrict__ A, long lda, int N, int K, int r, int rpad,
                                                         int tiles_per_block, float scale, int bvec) {
    extern __shared__ __align__(16) unsigned char smem[];
    float* red = (float*)smem;                                  // [LM_ROWS][LM_RED_LD]
    bf16* at = (bf16*)(smem + LM_ROWS * LM_RED_LD * 4);         // [LM_COLS][rpad + 8] (8-element pad: rows start on other banks)
    const int ld_at = rpad + 8;
    const int k0 = blockIdx.x * LM_COLS;
    const int lane = lane_id(), w = wave_id();
    for (int idx = threadIdx.x; idx < rpad * LM_COLS; idx += 256) {
        const int j = idx / LM_COLS, c = idx % LM_COLS;
        at[c * ld_at + j] = (j < r && k0 + c < K) ? A[(long)j * lda + k0 + c] : (bf16)0.f;
    }
    const int ks = rpad / 32;
    const int rt0 = blockIdx.y * tiles_per_block;
    const int rt1 = min(rt0 + tiles_per_block, (N + LM_ROWS - 1) / LM_ROWS);
    const int ec = (threadIdx.x & 7) * 8, er = threadIdx.x >> 3;     // epilogue: columns ec .. ec + 7 of rows er and er + 32
    const bool col_ok = k0 + ec < K;                                 // K % 8 == 0: the 8 columns are all in or all out
    for (int rt = rt0; rt < rt1; ++rt) {
        const int n0 = rt * LM_ROWS;
        bf16x8 wv[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int n = n0 + er + 32 * h;
            const bf16x8* p = (const bf16x8*)(W + (long)n * ldw + k0 + ec);
            wv[h] = (n < N && col_ok) ? (NT ? __builtin_nontemporal_load(p) : *p) : zero8();
        }
        const int nb = n0 + 16 * w + (lane & 15);
        const bf16* brow = B + (long)(nb < N ? nb : 0) * ldb;
        f32x4 acc[4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        __syncthreads();                       // the A strip is staged; the previous tile's epilogue is done with `red`
        for (int s = 0; s < ks; ++s) {
            const int j0 = 32 * s + 8 * (lane >> 4);
            bf16x8 bf = zero8();
            if (nb < N) {
                if (bvec) {                    // r % 8 == 0, ldb % 8 == 0, B 16-byte aligned: j0 < r means all 8 are in
                    if (j0 < r) bf = *(const bf16x8*)(brow + j0);
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (j0 + e < r) bf[e] = brow[j0 + e];
                }
            }
#pragma unroll
            for (int ct = 0; ct < 4; ++ct)
                acc[ct] = mfma16(bf, *(const bf16x8*)(at + (ct * 16 + (lane & 15)) * ld_at + j0), acc[ct]);
        }
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
            for (int i = 0; i < 4; ++i) red[(16 * w + 4 * (lane >> 4) + i) * LM_RED_LD + ct * 16 + (lane & 15)] = acc[ct][i];
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int n = n0 + er + 32 * h;
            if (n < N && col_ok) {
                const float* d = red + (er + 32 * h) * LM_RED_LD + ec;
                bf16x8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = f2bf(bf2f(wv[h][e]) + scale * d[e]);
                bf16x8* p = (bf16x8*)(W + (long)n * ldw + k0 + ec);
                if (NT)
                    __builtin_nontemporal_store(o, p);
                else
                    *p = o;
            }
        }
    }
}

}  // namespace

extern "C" int rv_lora_merge_bf16(void* W, int64_t ldw, const void* B, int64_t ldb, const void* A, int64_t lda, int N, int K, int r,
                                  float scale, void* stream) {
    if (!W || !B || !A || N <= 0 || K <= 0 || r < 1 || r > 256 || (K & 7) || (ldw & 7) || ldw < K || ldb < r || lda < K ||
        ((uintptr_t)W & 15))
        return RV_ERR_ARG;
    // W is read and written once: nontemporal loads and stores (MI355X_MICROARCH "nt-weights"), 8-9 % less time than the default
    // policy at 7B, 13B and Qwen2-7B (profiles/lora_merge_bench.jsonl).  RV_LORA_MERGE_NT=0 selects the default policy (A/B only).
    static const bool nt = [] { const char* e = getenv("RV_LORA_MERGE_NT"); return !(e && e[0] == '0'); }();
    const int rpad = (r + 31) / 32 * 32;
    const int bvec = (r % 8 == 0 && ldb % 8 == 0 && ((uintptr_t)B & 15) == 0) ? 1 : 0;
    const long xs = cdiv(K, LM_COLS), rts = cdiv(N, LM_ROWS);
    const int tpb = (int)((rts * xs + LM_BLOCKS - 1) / LM_BLOCKS);
    const dim3 grid((unsigned)xs, cdiv(rts, tpb));
    const size_t smem = (size_t)LM_ROWS * LM_RED_LD * 4 + (size_t)LM_COLS * (rpad + 8) * 2;
    if (nt)
        hipLaunchKernelGGL(lora_merge_kernel<true>, grid, dim3(256), smem, ST, (bf16*)W, (long)ldw, (const bf16*)B, (long)ldb,
                           (const bf16*)A, (long)lda, N, K, r, rpad, tpb, scale, bvec);
    else
        hipLaunchKernelGGL(lora_merge_kernel<false>, grid, dim3(256), smem, ST, (bf16*)W, (long)ldw, (const bf16*)B, (long)ldb,
                           (const bf16*)A, (long)lda, N, K, r, rpad, tpb, scale, bvec);
    return rv_check_launch();
}
