// Decoding with live LoRA adapters on gfx950: the first of the two launches a fused projection takes at M = 1..32 rows when its
// adapters are not merged.
//   rv_lora_down_rows_bf16   T[M, j r .. (j + 1) r) = bf16(scale * X A_j^T) for the up to three adapters that share the input X
// The second, rv_gemv_lora_bf16 (Y = X W^T + T_j B_j^T), is an instantiation of gemv_kernel and lives in gemv.hip.
// The down-projection keeps gemv.hip's rule: reductions in a fixed order that depends on the operand shapes only, never on M, on other
// rows or on timing, and no atomics -- a row's result is bit-identical whatever else shares its launch.
#include "common.h"
#include "radvlm_hip.h"

namespace {

constexpr int DOWN_U = 4;        // K steps in flight per wave
constexpr int LD_MODS = 3;

// ------------------------------------------------------------------------------------------------ down-projection, M <= 32
// Workgroup (x, y): 16 rows of one adapter A_j (x = j * ceil(r / 16) + tile), K slice y of rv_lora_down_split(r, K).  The slice's K steps
// (32 deep) are split into 4 contiguous runs, one per wave, as in gemv_kernel; A goes straight from HBM to VGPRs (dwordx4, nt: every
// adapter row is read once per call, by one workgroup), X (<= 32 rows, L2-resident) beside it.  MFMA 16x16x32: A operand = X rows,
// B operand = adapter rows (lane l: adapter row l & 15, k 8 (l >> 4) .. + 7) -> D[row][adapter row].  One slice: the sum is scaled,
// rounded and stored here; more: fp32 partials [slice][M][n_mod r], summed in slice order by down_combine_kernel.
struct DownMods {
    const bf16* a[LD_MODS];
};

template <int MT>
__global__ __launch_bounds__(256) void lora_down_rows_kernel(const bf16* __restrict__ X, long ldx, DownMods mods, long lda, int r, int M, int K,
                                                             int split, float scale, float* __restrict__ part, bf16* __restrict__ T, long ldt) {
    __shared__ float red[4][MT * 16][16];
    const int lane = lane_id(), w = wave_id();
    const int c = lane & 15, kg = lane >> 4;
    const int tiles = (r + 15) / 16;
    const int j = blockIdx.x / tiles, a0 = (blockIdx.x % tiles) * 16;
    const int sidx = blockIdx.y;
    const int ks = (K + 31) / 32;
    const int unit = sidx * 4 + w, units = split * 4;
    const int s0 = (int)((long)ks * unit / units), s1 = (int)((long)ks * (unit + 1) / units);
    const bf16* __restrict__ A = j == 0 ? mods.a[0] : (j == 1 ? mods.a[1] : mods.a[2]);
    const bool a_ok = a0 + c < r;
    const bf16* ap = A + (long)(a_ok ? a0 + c : 0) * lda + kg * 8;
    const bf16* xp[MT];
    bool m_ok[MT];
#pragma unroll
    for (int rt = 0; rt < MT; ++rt) {
        const int m = rt * 16 + c;
        m_ok[rt] = m < M;
        xp[rt] = X + (long)(m_ok[rt] ? m : 0) * ldx + kg * 8;
    }
    f32x4 acc[MT];
#pragma unroll
    for (int rt = 0; rt < MT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int st = s0; st < s1; st += DOWN_U) {
        bf16x8 af[DOWN_U], xf[DOWN_U][MT];
#pragma unroll
        for (int u = 0; u < DOWN_U; ++u) {
            const int k = (st + u) * 32;
            const bool kin = (st + u) < s1 && k + kg * 8 < K;           // K % 8 == 0: a lane's 8 elements are all in or all out
            af[u] = (kin && a_ok) ? ld_nt(ap + k) : zero8();
#pragma unroll
            for (int rt = 0; rt < MT; ++rt) xf[u][rt] = (kin && m_ok[rt]) ? *(const bf16x8*)(xp[rt] + k) : zero8();
        }
#pragma unroll
        for (int u = 0; u < DOWN_U; ++u)
#pragma unroll
            for (int rt = 0; rt < MT; ++rt) acc[rt] = mfma16(xf[u][rt], af[u], acc[rt]);
    }
#pragma unroll
    for (int rt = 0; rt < MT; ++rt)
#pragma unroll
        for (int q = 0; q < 4; ++q) red[w][rt * 16 + 4 * kg + q][c] = acc[rt][q];
    __syncthreads();
    const int nt = gridDim.x / tiles * r;                                // columns of T: n_mod * r
    for (int idx = threadIdx.x; idx < MT * 16 * 16; idx += 256) {
        const int m = idx / 16, col = idx % 16;
        if (m >= M || a0 + col >= r) continue;
        float v = red[0][m][col];
        v += red[1][m][col];
        v += red[2][m][col];
        v += red[3][m][col];
        const int n = j * r + a0 + col;
        if (split > 1)
            part[((long)sidx * M + m) * nt + n] = v;
        else
            T[(long)m * ldt + n] = f2bf(v * scale);
    }
}

__global__ void down_combine_kernel(const float* __restrict__ part, int split, int M, int nt, float scale, bf16* __restrict__ T, long ldt) {
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= (long)M * nt) return;
    const int m = (int)(tid / nt), n = (int)(tid % nt);
    float v = part[tid];
    for (int s = 1; s < split; ++s) v += part[(long)s * M * nt + tid];
    T[(long)m * ldt + n] = f2bf(v * scale);
}

}  // namespace

extern "C" int rv_lora_down_split(int r, int K) {
    // K slices per 16 adapter rows: the adapters are r <= 64 rows each, so only K gives workgroups; every wave keeps >= 2 of its 32-deep
    // K steps.  A function of K only (r is taken so that a later rule may use it): a row's reduction order never depends on M.
    (void)r;
    const long ks = (K + 31) / 32;
    int split = 1;
    while (split < 32 && ks >= (long)split * 2 * 4 * 2) split *= 2;
    return split;
}

extern "C" int rv_lora_down_rows_bf16(const void* X, int64_t ldx, const void* A0, const void* A1, const void* A2, int64_t lda, int n_mod, void* T,
                                      int64_t ldt, int M, int r, int K, float scale, void* workspace, int64_t ws_bytes, void* stream) {
    if (!X || !T || n_mod < 1 || n_mod > LD_MODS || M < 1 || M > 32 || !lora_rank_ok(r) || K <= 0 || (K & 7) || (ldx & 7) || ldx < K || (lda & 7) ||
        lda < K || ldt < (int64_t)n_mod * r || !aligned16(X))
        return RV_ERR_ARG;
    const void* a[LD_MODS] = {A0, A1, A2};
    DownMods mods;
    for (int j = 0; j < LD_MODS; ++j) {
        if (j < n_mod && (!a[j] || !aligned16(a[j]))) return RV_ERR_ARG;
        mods.a[j] = (const bf16*)(j < n_mod ? a[j] : a[0]);
    }
    const int split = rv_lora_down_split(r, K), nt = n_mod * r;
    float* part = nullptr;
    if (split > 1) {
        if (!workspace || ws_bytes < (int64_t)split * M * nt * 4) return RV_ERR_ARG;
        part = (float*)workspace;
    }
    const dim3 grid(n_mod * cdiv(r, 16), split);
    if (M <= 16)
        hipLaunchKernelGGL(lora_down_rows_kernel<1>, grid, dim3(256), 0, ST, (const bf16*)X, (long)ldx, mods, (long)lda, r, M, K, split, scale, part,
                           (bf16*)T, (long)ldt);
    else
        hipLaunchKernelGGL(lora_down_rows_kernel<2>, grid, dim3(256), 0, ST, (const bf16*)X, (long)ldx, mods, (long)lda, r, M, K, split, scale, part,
                           (bf16*)T, (long)ldt);
    if (split > 1)
        hipLaunchKernelGGL(down_combine_kernel, dim3(cdiv((long)M * nt, 256)), dim3(256), 0, ST, (const float*)part, split, M, nt, scale, (bf16*)T,
                           (long)ldt);
    return rv_check_launch();
}
