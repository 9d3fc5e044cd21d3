// Prompt-lookup (speculative) decoding kernel for gfx950: decode attention of R consecutive query rows of one sequence -- the last
// emitted token and R - 1 drafted ones, row i seeing the keys [0, kv_len0 + i) -- with every K / V fragment of a chunk loaded and
// converted once for a whole group of rows.  As in decode.hip every reduction runs in a fixed order that depends on the row's own key
// count only and there are no global or float atomics: a row's result is bit-identical to rv_attn_decode_bf16 on that row alone.
// Reference call sites are listed per entry point in include/radvlm_hip.h.
#include "attn_split.h"
#include "common.h"
#include "radvlm_hip.h"

#include <math.h>

namespace {

// ------------------------------------------------------------------------------------------------ verify decode attention
// decode.hip's attn_decode_kernel for a staircase of rows.  Block (chunk c, kv head kh, sequence b x row group): a "query" is one
// (row, q head of kv head kh) pair, up to AD_NQ = 16 of them per block (rows per group = 16 / G: 16 rows of an MHA model, 2 of a G = 7
// or 8 one), query nq = (row - first row) * G + g.  Query nq sees the chunk's first nr[nq] keys, nr = min(j0 + chunk, len_row) - j0 with
// len_row = min(kv_len0[b] + row, L_max); only the last one or two chunks differ between the rows of a group.
// This kernel is the prologue (the key counts and the q rows, to LDS); the rest is attn_split.h's attn_decode_nq_body, where the list
// of what keeps a row's bits those of attn_decode_kernel at kv_len = kv_len0[b] + row stands.  The combine runs with the row's own
// key count (RowsStair).
constexpr int AV_RMAX = 32;

template <int HD>
__global__ __launch_bounds__(256) void attn_decode_verify_kernel(const bf16* __restrict__ q, long ld_q, const bf16* __restrict__ cache, long ld_c,
                                                                 long bs_c, int v_off, const int* __restrict__ kv_len0, int L_max,
                                                                 float* __restrict__ part, int R, int rpg, int H, int Hkv, int chunk, float scale) {
    constexpr int LPR = HD / 8;
    __shared__ float buf[AD_NQ_BUF<HD>];        // sc[AD_NQ][chunk] through the P V loop, then ored[4][AD_NQ][HD]
    __shared__ float qs[AD_NQ][HD];
    __shared__ int nrs[AD_NQ];
    const int c = blockIdx.x, kh = blockIdx.y;
    const int ngrp = (R + rpg - 1) / rpg;
    const int b = blockIdx.z / ngrp, r0 = (blockIdx.z % ngrp) * rpg;
    const int G = H / Hkv;
    const int rows = min(rpg, R - r0), NQ = rows * G;
    const int kv0 = kv_len0[b];
    const int j0 = c * chunk;
    const int len_max = min(kv0 + r0 + rows - 1, L_max);          // the group's last row sees the most keys
    if (j0 >= len_max) return;                  // no row of the group reaches this chunk; the combine reads a row's own chunks only
    const int j1 = min(j0 + chunk, len_max);
    const bf16* kbase = cache + (long)b * bs_c + kh * HD + lane_id() % LPR * 8;
    if (threadIdx.x < AD_NQ) {
        const int nq = threadIdx.x;
        int n = 0;
        if (nq < NQ) n = min(max(min(j0 + chunk, min(kv0 + r0 + nq / G, L_max)) - j0, 0), chunk);
        nrs[nq] = n;
    }
    for (int idx = threadIdx.x; idx < NQ * LPR; idx += 256) {
        const int nq = idx / LPR, s = idx % LPR;
        const bf16x8 t = *(const bf16x8*)(q + ((long)b * R + r0 + nq / G) * ld_q + (kh * G + nq % G) * HD + s * 8);
#pragma unroll
        for (int i = 0; i < 8; ++i) qs[nq][s * 8 + i] = bf2f(t[i]);
    }
    __syncthreads();
    attn_decode_nq_body<HD>(kbase, kbase + v_off, ld_c, buf, qs, nrs, NQ, [=](int nq) { return (long)b * R + r0 + nq / G; }, j0, j1, part, H, G,
                            chunk, scale);
}

}  // namespace

extern "C" int rv_attn_decode_verify_bf16(const void* q, int64_t ld_q, const void* cache, int64_t ld_c, int64_t bs_c, int v_off,
                                          const int32_t* kv_len0, int L_max, void* out, int64_t ld_o, void* part, int64_t part_bytes, int B,
                                          int R, int H, int Hkv, int hd, int chunk, float scale, void* stream) {
    const bool ok = kv_len0 && B > 0 && R >= 1 && R <= AV_RMAX && ad_chunk_ok(chunk, hd) && split_cache_ok(cache, ld_c, bs_c, v_off, Hkv, hd, L_max);
    return attn_split_launch(ok, q, ld_q, out, ld_o, part, part_bytes, (int64_t)B * R, H, Hkv, hd, L_max, chunk, stream,
                             RowsStair{kv_len0, L_max, R}, [&](auto hd_c, int nch) {
                                 const int rpg = AD_NQ / (H / Hkv);          // rows per block: G <= 8, so at least 2
                                 const int ngrp = (R + rpg - 1) / rpg;
                                 hipLaunchKernelGGL(attn_decode_verify_kernel<hd_c()>, dim3(nch, Hkv, B * ngrp), dim3(256), 0, ST, (const bf16*)q,
                                                    (long)ld_q, (const bf16*)cache, (long)ld_c, (long)bs_c, v_off, kv_len0, L_max, (float*)part, R,
                                                    rpg, H, Hkv, chunk, scale);
                             });
}
