// Shared-prefix decode attention for gfx950: rv_attn_decode_bf16 for a batch in which groups of cache rows ("tiles") hold bit-equal K|V
// at their first c0 * chunk positions -- the requests of one generate_batch() call that begin with the same image and system prompt.
// A shared chunk's K / V fragments are loaded and converted once, from the tile's first row, for every (row, q head) query of the tile;
// a chunk at or past c0 is the plain kernel's work on the row alone.  As in decode.hip every reduction runs in a fixed order that depends
// on the row's own key count only and there are no global or float atomics: a row's result is bit-identical to rv_attn_decode_bf16 on
// the same cache.  Reference call sites are listed per entry point in include/radvlm_hip.h.
#include "attn_split.h"
#include "common.h"
#include "radvlm_hip.h"

#include <math.h>

namespace {

// ------------------------------------------------------------------------------------------------ shared-prefix decode attention
// decode.hip's attn_decode_kernel restated the way lookup.hip restates it for a staircase.  Block (chunk c, kv head kh, row b), grid
// (nch, Hkv, B) as there.  A "query" is one (row, q head of kv head kh) pair, up to AS_NQ = 16 of them per block:
//   c >= c0[b]: the block's rows are {b}, its G queries the plain kernel's;
//   c <  c0[b]: the block returns at once unless b leads its tile (tile[b][0] == b); a leading block's rows are tile[b][0 .. 16 / G)
//               up to the first -1, query nq = t * G + g for the tile's t-th row, and every K / V fragment is read from row b.
// Query nq sees the chunk's first nr[nq] keys, nr = min(j0 + chunk, len_row) - j0 with len_row = min(kv_len[row], L_max), in a shared
// chunk capped by the leading row's own count: a position at or past a row's kv_len (its own or the leader's) never reaches an output,
// whatever the table says.  Rows outside [0, B) end the list.  Under the contract (every row of a tile holds c0 * chunk keys or more)
// nr is `chunk` for every query of a shared chunk.
// This kernel is the prologue (the rows, their key counts and q rows, to LDS); the rest is attn_split.h's attn_decode_nq_body, as for
// lookup.hip's staircase, where the list of what keeps a row's bits those of attn_decode_kernel stands.  The K / V bits come from the
// leading row instead of the row's own: equal by the contract.  The combine is the plain kernel's (RowsKvLen).
constexpr int AS_NQ = AD_NQ;
constexpr int AS_TILE = 16;                     // columns of the tile table

template <int HD>
__global__ __launch_bounds__(256) void attn_decode_shared_kernel(const bf16* __restrict__ q, long ld_q, const bf16* __restrict__ cache, long ld_c,
                                                                 long bs_c, int v_off, const int* __restrict__ kv_len,
                                                                 const int* __restrict__ c0v, const int* __restrict__ tile, int L_max,
                                                                 float* __restrict__ part, int B, int H, int Hkv, int chunk, float scale) {
    constexpr int LPR = HD / 8;
    __shared__ float buf[AD_NQ_BUF<HD>];        // sc[AS_NQ][chunk] through the P V loop, then ored[4][AS_NQ][HD]
    __shared__ float qs[AS_NQ][HD];
    __shared__ int nrs[AS_NQ];
    __shared__ int rws[AS_NQ];                  // cache / q / part row of each query, -1: none
    const int c = blockIdx.x, kh = blockIdx.y, b = blockIdx.z;
    const int G = H / Hkv, rpt = AS_NQ / G;
    const bool shared = c < c0v[b];
    if (shared && tile[(long)b * AS_TILE] != b) return;           // the tile's leading block writes this row's partial
    const int len_b = min(kv_len[b], L_max);
    const int j0 = c * chunk;
    if (j0 >= len_b) return;                    // as the plain kernel; a shared chunk holds at most the leading row's keys
    const int j1 = min(j0 + chunk, len_b);
    const bf16* kbase = cache + (long)b * bs_c + kh * HD + lane_id() % LPR * 8;
    if (threadIdx.x < AS_NQ) {
        const int nq = threadIdx.x, t = nq / G;
        int row = -1;
        if (t == 0) {
            row = b;
        } else if (shared && t < rpt) {
            row = b;                            // walk the list: a -1 or an out-of-range entry ends it
            for (int k = 1; k <= t && row >= 0; ++k) {
                const int e = tile[(long)b * AS_TILE + k];
                row = (e >= 0 && e < B) ? e : -1;
            }
        }
        int n = 0;
        if (row >= 0 && nq < rpt * G) n = min(max(min(j1, min(kv_len[row], L_max)) - j0, 0), chunk);
        nrs[nq] = n;
        rws[nq] = n > 0 ? row : -1;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < AS_NQ * LPR; idx += 256) {
        const int nq = idx / LPR, s = idx % LPR;
        const int row = rws[nq];
        if (row < 0) continue;
        const bf16x8 t = *(const bf16x8*)(q + (long)row * ld_q + (kh * G + nq % G) * HD + s * 8);
#pragma unroll
        for (int i = 0; i < 8; ++i) qs[nq][s * 8 + i] = bf2f(t[i]);
    }
    __syncthreads();
    attn_decode_nq_body<HD>(kbase, kbase + v_off, ld_c, buf, qs, nrs, AS_NQ, [&](int nq) { return (long)rws[nq]; }, j0, j1, part, H, G, chunk,
                            scale);
}

}  // namespace

extern "C" int rv_attn_decode_shared_bf16(const void* q, int64_t ld_q, const void* cache, int64_t ld_c, int64_t bs_c, int v_off,
                                          const int32_t* kv_len, const int32_t* c0, const int32_t* tile, int L_max, void* out, int64_t ld_o,
                                          void* part, int64_t part_bytes, int B, int H, int Hkv, int hd, int chunk, float scale, void* stream) {
    const bool ok = kv_len && c0 && tile && ad_chunk_ok(chunk, hd) && split_cache_ok(cache, ld_c, bs_c, v_off, Hkv, hd, L_max);
    return attn_split_launch(ok, q, ld_q, out, ld_o, part, part_bytes, B, H, Hkv, hd, L_max, chunk, stream, RowsKvLen{kv_len, L_max},
                             [&](auto hd_c, int nch) {
                                 hipLaunchKernelGGL(attn_decode_shared_kernel<hd_c()>, dim3(nch, Hkv, B), dim3(256), 0, ST, (const bf16*)q,
                                                    (long)ld_q, (const bf16*)cache, (long)ld_c, (long)bs_c, v_off, kv_len, c0, tile, L_max,
                                                    (float*)part, B, H, Hkv, chunk, scale);
                             });
}
