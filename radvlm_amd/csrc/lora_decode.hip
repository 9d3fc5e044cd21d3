// Decoding with live LoRA adapters on gfx950: the two launches a fused projection takes at M = 1..32 rows when its adapters are not merged.
//   rv_lora_down_rows_bf16   T[M, j r .. (j + 1) r) = bf16(scale * X A_j^T) for the up to three adapters that share the input X
//   rv_gemv_lora_bf16        Y = X W^T + T_j B_j^T (+ bias) (+ residual): rv_gemv_bf16 (gemv.hip) with the adapter as extra K steps
// Both keep gemv.hip's rule: reductions in a fixed order that depends on the operand shapes only, never on M, on other rows or on timing,
// and no atomics -- a row's result is bit-identical whatever else shares its launch.
// rv_gemv_lora_bf16 restates gemv_kernel's bf16 body instead of sharing it: gemv.hip's note on its parameter pack records that moving
// that body changes the register allocation of the kernels every decode step runs, and those stay instruction for instruction as they are.
#include "common.h"
#include "radvlm_hip.h"

#include <type_traits>

namespace {

constexpr int LD_COLS = 64;      // output columns per workgroup of the fused kernel (gemv.hip's GV_COLS)
constexpr int LD_U = 4;          // K steps in flight per wave (gemv.hip's GV_U)
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
    for (int st = s0; st < s1; st += LD_U) {
        bf16x8 af[LD_U], xf[LD_U][MT];
#pragma unroll
        for (int u = 0; u < LD_U; ++u) {
            const int k = (st + u) * 32;
            const bool kin = (st + u) < s1 && k + kg * 8 < K;           // K % 8 == 0: a lane's 8 elements are all in or all out
            af[u] = (kin && a_ok) ? ld_nt(ap + k) : zero8();
#pragma unroll
            for (int rt = 0; rt < MT; ++rt) xf[u][rt] = (kin && m_ok[rt]) ? *(const bf16x8*)(xp[rt] + k) : zero8();
        }
#pragma unroll
        for (int u = 0; u < LD_U; ++u)
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

// ------------------------------------------------------------------------------------------------ skinny NT GEMM with the adapter
// gemv_kernel's bf16 instantiation (gemv.hip: block of 4 waves and 64 columns, the K steps of the block's slice in 4 contiguous runs,
// W as nontemporal dwordx4 loads, LD_U steps in flight, ascending step order per accumulator, the four-wave LDS sum, the epilogue), and
// after its K loop the adapter: wave 0 of slice 0 runs ceil(r / 32) more steps into the same accumulators with T in X's place
// (columns toff .. toff + r of T) and the block's rows of B_j in W's.  Every product of a zero B is a zero, so with B = 0 the
// accumulators, and every bit of Y, are rv_gemv_bf16's.  T and B are a few KB, read by every column block: plain loads, L2-resident.
// A 64-column block lies in at most one module (boundaries are multiples of 64; the launcher checks), so the module is block-uniform.
struct UpMods {
    const bf16* b[LD_MODS];
    int c0[LD_MODS], c1[LD_MODS], toff[LD_MODS];
};

template <int MT>
__global__ __launch_bounds__(256) void gemv_lora_kernel(const bf16* __restrict__ X, long ldx, const bf16* __restrict__ W, long ldw,
                                                        const bf16* __restrict__ T, long ldt, UpMods mods, int n_mod, long ldb, int r, int M, int N,
                                                        int K, int split, float* __restrict__ part, bf16* __restrict__ Y, long ldy,
                                                        const bf16* __restrict__ bias, const bf16* __restrict__ R, long ldr) {
    __shared__ float red[4][MT * 16][LD_COLS];
    const int lane = lane_id(), w = wave_id();
    const int c = lane & 15, kg = lane >> 4;
    const int n0 = blockIdx.x * LD_COLS;
    const int sidx = blockIdx.y;
    const int ks = (K + 31) / 32;
    const int unit = sidx * 4 + w, units = split * 4;
    const int s0 = (int)((long)ks * unit / units), s1 = (int)((long)ks * (unit + 1) / units);
    const bf16* wp[4];
    bool n_ok[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        const int n = n0 + ct * 16 + c;
        n_ok[ct] = n < N;
        wp[ct] = W + (long)(n_ok[ct] ? n : 0) * ldw + kg * 8;
    }
    const bf16* xp[MT];
    bool m_ok[MT];
#pragma unroll
    for (int rt = 0; rt < MT; ++rt) {
        const int m = rt * 16 + c;
        m_ok[rt] = m < M;
        xp[rt] = X + (long)(m_ok[rt] ? m : 0) * ldx + kg * 8;
    }
    f32x4 acc[MT][4];
#pragma unroll
    for (int rt = 0; rt < MT; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int st = s0; st < s1; st += LD_U) {
        bf16x8 wf[LD_U][4], xf[LD_U][MT];
#pragma unroll
        for (int u = 0; u < LD_U; ++u) {
            const int k = (st + u) * 32;
            const bool kin = (st + u) < s1 && k + kg * 8 < K;           // K % 8 == 0: a lane's 8 elements are all in or all out
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) wf[u][ct] = (kin && n_ok[ct]) ? ld_nt(wp[ct] + k) : zero8();
#pragma unroll
            for (int rt = 0; rt < MT; ++rt) xf[u][rt] = (kin && m_ok[rt]) ? *(const bf16x8*)(xp[rt] + k) : zero8();
        }
#pragma unroll
        for (int u = 0; u < LD_U; ++u)
#pragma unroll
            for (int rt = 0; rt < MT; ++rt)
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = mfma16(xf[u][rt], wf[u][ct], acc[rt][ct]);
    }
    if (unit == 0) {                                                     // wave-uniform: the adapter's steps, after all of this wave's W steps
        int j = -1;
#pragma unroll
        for (int i = 0; i < LD_MODS; ++i)
            if (i < n_mod && n0 >= mods.c0[i] && n0 < mods.c1[i]) j = i;
        if (j >= 0) {
            const bf16* __restrict__ Bj = j == 0 ? mods.b[0] : (j == 1 ? mods.b[1] : mods.b[2]);
            const int c0 = j == 0 ? mods.c0[0] : (j == 1 ? mods.c0[1] : mods.c0[2]);
            const int c1 = j == 0 ? mods.c1[0] : (j == 1 ? mods.c1[1] : mods.c1[2]);
            const int toff = j == 0 ? mods.toff[0] : (j == 1 ? mods.toff[1] : mods.toff[2]);
            for (int k = 0; k < r; k += 32) {
                const bool kin = k + kg * 8 < r;                         // r % 8 == 0
                bf16x8 bfr[4], tf[MT];
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    const int n = n0 + ct * 16 + c;
                    bfr[ct] = (kin && n < c1) ? *(const bf16x8*)(Bj + (long)(n - c0) * ldb + k + kg * 8) : zero8();
                }
#pragma unroll
                for (int rt = 0; rt < MT; ++rt)
                    tf[rt] = (kin && m_ok[rt]) ? *(const bf16x8*)(T + (long)(rt * 16 + c) * ldt + toff + k + kg * 8) : zero8();
#pragma unroll
                for (int rt = 0; rt < MT; ++rt)
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = mfma16(tf[rt], bfr[ct], acc[rt][ct]);
            }
        }
    }
#pragma unroll
    for (int rt = 0; rt < MT; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
            for (int q = 0; q < 4; ++q) red[w][rt * 16 + 4 * kg + q][ct * 16 + c] = acc[rt][ct][q];
    __syncthreads();
    for (int idx = threadIdx.x; idx < MT * 16 * LD_COLS; idx += 256) {
        const int m = idx / LD_COLS, col = idx % LD_COLS, n = n0 + col;
        if (m >= M || n >= N) continue;
        float v = red[0][m][col];
        v += red[1][m][col];
        v += red[2][m][col];
        v += red[3][m][col];
        if (split > 1) {
            part[((long)sidx * M + m) * N + n] = v;
            continue;
        }
        if (bias) v += bf2f(bias[n]);
        if (R) v += bf2f(R[(long)m * ldr + n]);
        Y[(long)m * ldy + n] = f2bf(v);
    }
}

// split-K combine: gemv.hip's, bf16 output only
__global__ void gemv_lora_combine_kernel(const float* __restrict__ part, int split, int M, int N, bf16* __restrict__ Y, long ldy,
                                         const bf16* __restrict__ bias, const bf16* __restrict__ R, long ldr) {
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= (long)M * N) return;
    const int m = (int)(tid / N), n = (int)(tid % N);
    float v = part[tid];
    for (int s = 1; s < split; ++s) v += part[(long)s * M * N + tid];
    if (bias) v += bf2f(bias[n]);
    if (R) v += bf2f(R[(long)m * ldr + n]);
    Y[(long)m * ldy + n] = f2bf(v);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool rank_ok(int r) { return r >= 8 && r <= 64 && !(r & 7); }     // the ranks the training path accepts

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
    if (!X || !T || n_mod < 1 || n_mod > LD_MODS || M < 1 || M > 32 || !rank_ok(r) || K <= 0 || (K & 7) || (ldx & 7) || ldx < K || (lda & 7) ||
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

extern "C" int rv_gemv_lora_bf16(const void* X, int64_t ldx, const void* W, int64_t ldw, const void* T, int64_t ldt, int r, int n_mod,
                                 const void* B0, int col0_0, int col1_0, int toff0, const void* B1, int col0_1, int col1_1, int toff1, const void* B2,
                                 int col0_2, int col1_2, int toff2, int64_t ldb, void* Y, int64_t ldy, const void* bias, const void* residual,
                                 int64_t ldr, int M, int N, int K, void* workspace, int64_t ws_bytes, void* stream) {
    if (!X || !W || !T || !Y || M < 1 || M > 32 || N <= 0 || K <= 0 || (K & 7) || (ldx & 7) || ldx < K || (ldw & 7) || ldw < K || ldy < N ||
        (residual && ldr < N) || !rank_ok(r) || n_mod < 1 || n_mod > LD_MODS || (ldt & 7) || (ldb & 7) || ldb < r || !aligned16(X) ||
        !aligned16(W) || !aligned16(T))
        return RV_ERR_ARG;
    const void* b[LD_MODS] = {B0, B1, B2};
    const int c0[LD_MODS] = {col0_0, col0_1, col0_2}, c1[LD_MODS] = {col1_0, col1_1, col1_2}, to[LD_MODS] = {toff0, toff1, toff2};
    UpMods mods;
    int prev = 0;
    for (int j = 0; j < LD_MODS; ++j) {
        if (j < n_mod) {
            // ascending, disjoint column ranges; a boundary inside Y is a multiple of 64 (a column block never straddles two modules)
            if (!b[j] || !aligned16(b[j]) || c0[j] < prev || c1[j] <= c0[j] || c1[j] > N || (c0[j] % LD_COLS) || (c1[j] != N && (c1[j] % LD_COLS)) ||
                to[j] < 0 || (to[j] & 7) || (int64_t)to[j] + r > ldt)
                return RV_ERR_ARG;
            prev = c1[j];
        }
        mods.b[j] = (const bf16*)(j < n_mod ? b[j] : b[0]);
        mods.c0[j] = j < n_mod ? c0[j] : 0;
        mods.c1[j] = j < n_mod ? c1[j] : 0;
        mods.toff[j] = j < n_mod ? to[j] : 0;
    }
    const int split = rv_gemv_split(N, K);
    float* part = nullptr;
    if (split > 1) {
        if (!workspace || ws_bytes < (int64_t)split * M * N * 4) return RV_ERR_ARG;
        part = (float*)workspace;
    }
    const dim3 grid(cdiv(N, LD_COLS), split);
    if (M <= 16)
        hipLaunchKernelGGL(gemv_lora_kernel<1>, grid, dim3(256), 0, ST, (const bf16*)X, (long)ldx, (const bf16*)W, (long)ldw, (const bf16*)T,
                           (long)ldt, mods, n_mod, (long)ldb, r, M, N, K, split, part, (bf16*)Y, (long)ldy, (const bf16*)bias, (const bf16*)residual,
                           (long)ldr);
    else
        hipLaunchKernelGGL(gemv_lora_kernel<2>, grid, dim3(256), 0, ST, (const bf16*)X, (long)ldx, (const bf16*)W, (long)ldw, (const bf16*)T,
                           (long)ldt, mods, n_mod, (long)ldb, r, M, N, K, split, part, (bf16*)Y, (long)ldy, (const bf16*)bias, (const bf16*)residual,
                           (long)ldr);
    if (split > 1)
        hipLaunchKernelGGL(gemv_lora_combine_kernel, dim3(cdiv((long)M * N, 256)), dim3(256), 0, ST, (const float*)part, split, M, N, (bf16*)Y,
                           (long)ldy, (const bf16*)bias, (const bf16*)residual, (long)ldr);
    return rv_check_launch();
}
