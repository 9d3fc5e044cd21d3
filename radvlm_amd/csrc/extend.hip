// Extend attention for gfx950: the prompt pass of a continued generate() call, causal attention of the uncached suffix rows of each
// sequence against that sequence's KV cache (the reused prefix plus the suffix's own rows, already written).  Query i of sequence b sits
// at position r[b] + i and attends to the keys [0, r[b] + i].
//
// Work split, flash-decoding style: block (chunk c, kv head kh, query tile z) takes the keys [c*chunk, (c+1)*chunk) of one tile of
// XT_QS * 16 query rows of one sequence times the G = H / Hkv query heads of kv head kh, so every K / V tile staged in LDS feeds all of
// them; chunks past the tile's last key are skipped.  Each block writes the (unnormalised o, running max m, sum l) of its rows per chunk;
// attn_split_combine_kernel merges a row's chunks in chunk order.  Tiles start at each sequence's first suffix row and the chunk grid is
// fixed in absolute key positions, so a row's result depends on its own sequence only: bit-identical alone or in any batch.
// Reference call sites are listed in include/radvlm_hip.h.
#include "attn_split.h"
#include "common.h"
#include "radvlm_hip.h"

#include <math.h>

namespace {

// attn_split.h's MFMA body on one cache: key j of sequence b is position j of cache row b
template <int HD>
__global__ __launch_bounds__(256) void attn_extend_kernel(const bf16* __restrict__ q, long ld_q, const bf16* __restrict__ cache, long ld_c,
                                                          long bs_c, int v_off, const int* __restrict__ cu_q, const int* __restrict__ rr,
                                                          int L_max, float* __restrict__ part, int H, int Hkv, int chunk, int nch, int tiles,
                                                          float scale) {
    const int b = blockIdx.z / tiles;
    const int q_beg = cu_q[b], n_b = cu_q[b + 1] - q_beg, r0 = rr[b];
    const bf16* cb = cache + (long)b * bs_c + blockIdx.y * HD;
    attn_extend_body<HD>(q, ld_q, [=](int j) { return cb + (long)j * ld_c; }, v_off, q_beg, n_b, r0, L_max, part, H, Hkv, chunk, nch, tiles,
                         scale);
}

}  // namespace

extern "C" int rv_attn_extend_bf16(const void* q, int64_t ld_q, const void* cache, int64_t ld_c, int64_t bs_c, int v_off, const int32_t* cu_q,
                                   const int32_t* r, int L_max, void* out, int64_t ld_o, void* part, int64_t part_bytes, int B, int M, int max_q,
                                   int H, int Hkv, int hd, int chunk, float scale, void* stream) {
    const int tiles = xt_tiles(B, max_q, H, Hkv);
    const bool ok = cu_q && r && tiles > 0 && max_q <= M && chunk % XT_KT == 0 && split_cache_ok(cache, ld_c, bs_c, v_off, Hkv, hd, L_max);
    return attn_split_launch(ok, q, ld_q, out, ld_o, part, part_bytes, M, H, Hkv, hd, L_max, chunk, stream, RowsExtend{cu_q, r, B},
                             [&](auto hd_c, int nch) {
                                 hipLaunchKernelGGL(attn_extend_kernel<hd_c()>, dim3(nch, Hkv, B * tiles), dim3(256), 0, ST, (const bf16*)q,
                                                    (long)ld_q, (const bf16*)cache, (long)ld_c, (long)bs_c, v_off, cu_q, r, L_max, (float*)part, H,
                                                    Hkv, chunk, nch, tiles, scale);
                             });
}
