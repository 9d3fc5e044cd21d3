// 8-bit AdamW state (--optim adamw_bnb_8bit): block-wise dynamic quantisation of exp_avg / exp_avg_sq, 256 elements per block, one fp32
// absmax per block and state, two 256-entry codebooks (adam8_codebook.h).  The rule is stated in tests/adam8_ref.py; these kernels are
// held to it bit for bit.  One wave owns one block, four consecutive elements per lane: the block maximum is a cross-lane reduction
// (no LDS round trip, no barrier after the tables are staged), and a maximum is order-free, so every result is deterministic.
#include "common.h"
#define RV_ADAM8_TABLE __device__ const
#include "adam8_codebook.h"
#include "adamw_update.h"
#include "radvlm_hip.h"

#define A8_BLOCK 256
#define A8_WAVES 4                 // waves (= blocks of the format) per workgroup

// LDS copy of one or both codebooks and their midpoints: mid[i] = fp32((float64(q[i]) + float64(q[i + 1])) / 2) (the sum of two floats is
// exact in float64, so is its half: one rounding)
struct A8Tables {
    float q[2][256];
    float mid[2][256];             // 255 used
};
DEVINL void a8_stage_tables(A8Tables& t) {
    for (int i = threadIdx.x; i < 512; i += blockDim.x) {
        const int k = i >> 8, j = i & 255;
        const uint32_t* src = k ? rv_adam8_unsigned_bits : rv_adam8_signed_bits;
        const float a = __uint_as_float(src[j]);
        t.q[k][j] = a;
        t.mid[k][j] = j < 255 ? (float)(((double)a + (double)__uint_as_float(src[j + 1])) * 0.5) : 0.f;
    }
    __syncthreads();
}
// number of midpoints strictly below a (np.searchsorted(mid, a, side="left")): eight halvings over the 255 sorted midpoints
DEVINL int a8_code(const float* mid, float a) {
    int c = 0;
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) c += mid[c + s - 1] < a ? s : 0;
    return c;
}
// Quantise the lane's four values (lanes / elements beyond the block hold 0 and `valid` masks them): returns the block's absmax and
// writes the codes of the valid elements into `codes` (one byte each; the other bytes keep what `codes` held).
DEVINL float a8_quant4(const A8Tables& t, int kind, const float x[4], int valid, unsigned& codes) {
    float mx = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) mx = fmaxf(mx, kind ? x[j] : fabsf(x[j]));
    const float am = wave_max(mx);
    const float s = am != 0.f ? am : 1.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int c = a8_code(t.mid[kind], x[j] / s);
        if (kind && x[j] > 0.f && c == 0) c = 1;             // the guard: a positive exp_avg_sq never dequantises to 0
        if (j < valid) codes = (codes & ~(0xFFu << (8 * j))) | ((unsigned)c << (8 * j));
    }
    return am;
}

// ------------------------------------------------------------------------------------------------ one tensor: quantise / dequantise
__global__ __launch_bounds__(64 * A8_WAVES) void adam8_quantize_kernel(const float* x, long n, uint8_t* codes, float* absmax, int kind, long nblk) {
    __shared__ A8Tables t;
    a8_stage_tables(t);
    const long b = (long)blockIdx.x * A8_WAVES + wave_id();
    if (b >= nblk) return;
    const long e0 = b * A8_BLOCK + lane_id() * 4;
    const int valid = (int)(n - e0 < 4 ? (n - e0 < 0 ? 0 : n - e0) : 4);
    float xv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) xv[j] = j < valid ? x[e0 + j] : 0.f;
    unsigned c = 0;
    const float am = a8_quant4(t, kind, xv, valid, c);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < valid) codes[e0 + j] = (uint8_t)(c >> (8 * j));
    if (lane_id() == 0) absmax[b] = am;
}
__global__ __launch_bounds__(256) void adam8_dequantize_kernel(const uint8_t* codes, const float* absmax, long n, int kind, float* x) {
    __shared__ A8Tables t;
    a8_stage_tables(t);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        x[i] = __fmul_rn(t.q[kind][codes[i]], absmax[i / A8_BLOCK]);
}

// ------------------------------------------------------------------------------------------------ the fused step
// Block b of the slice belongs to the tensor t with tab[2][t] <= b < tab[2][t + 1] (tab: int64 [3, T] = start, length, first block);
// its elements are start + 256 (b - first) ... in p / master / g, its codes are bytes [256 b, 256 b + 256) of cm / cv (a short last
// block leaves the rest of its 256 bytes as they were), its scales am[b] / av[b].  A block whose first element is 4-aligned and
// that is full takes vector accesses (8 B gradient, 16 B master, 8 B parameter); any other takes scalar ones, masked past its end.
__global__ __launch_bounds__(64 * A8_WAVES) void adamw8_kernel(bf16* p, float* master, const bf16* g, uint8_t* cm, uint8_t* cv, float* am, float* av,
                                                               const long* tab, int T, long nblk, float lr, float b1, float b2, float eps,
                                                               float wd, float bc1, float bc2, const float* gscale) {
    __shared__ A8Tables t;
    a8_stage_tables(t);
    const long b = (long)blockIdx.x * A8_WAVES + wave_id();
    if (b >= nblk) return;
    int lo = 0, hi = T;                                      // wave-uniform: the last tensor whose first block is <= b
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab[2 * (long)T + mid] <= b) lo = mid; else hi = mid;
    }
    const long within = (b - tab[2 * (long)T + lo]) * A8_BLOCK;
    const long left = tab[(long)T + lo] - within;            // elements of the tensor from this block's first on (> 0 by the table)
    const long e0 = tab[lo] + within + lane_id() * 4;
    const long mine = left - lane_id() * 4;
    const int valid = (int)(mine < 4 ? (mine < 0 ? 0 : mine) : 4);
    const bool vec = left >= A8_BLOCK && !((tab[lo] + within) & 3);

    const float gs = gscale ? gscale[0] : 1.f;
    const float rs2 = rsqrtf(bc2);
    const float step = lr / bc1;
    const float decay = fmaf(-lr, wd, 1.f);

    float pp[4], gg[4];
    if (vec) {
        const bf16x4 gv = *(const bf16x4*)(g + e0);
        const f32x4 pv = *(const f32x4*)(master + e0);
#pragma unroll
        for (int j = 0; j < 4; ++j) { pp[j] = pv[j]; gg[j] = bf2f(gv[j]); }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            pp[j] = j < valid ? master[e0 + j] : 0.f;
            gg[j] = j < valid ? bf2f(g[e0 + j]) : 0.f;
        }
    }
    const long cb = b * A8_BLOCK + lane_id() * 4;
    unsigned cmw = *(const unsigned*)(cm + cb), cvw = *(const unsigned*)(cv + cb);
    const float sm = am[b], sv = av[b];
    float mm[4], vv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        mm[j] = __fmul_rn(t.q[0][(cmw >> (8 * j)) & 255], sm);
        vv[j] = __fmul_rn(t.q[1][(cvw >> (8 * j)) & 255], sv);
        if (j < valid) adamw_update(pp[j], mm[j], vv[j], gg[j] * gs, decay, step, b1, b2, rs2, eps);
        else { mm[j] = 0.f; vv[j] = 0.f; }
    }
    if (vec) {
        f32x4 pv;
        bf16x4 po;
#pragma unroll
        for (int j = 0; j < 4; ++j) { pv[j] = pp[j]; po[j] = f2bf(pp[j]); }
        *(f32x4*)(master + e0) = pv;
        *(bf16x4*)(p + e0) = po;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < valid) { master[e0 + j] = pp[j]; p[e0 + j] = f2bf(pp[j]); }
    }
    const float nm = a8_quant4(t, 0, mm, valid, cmw);
    const float nv = a8_quant4(t, 1, vv, valid, cvw);
    *(unsigned*)(cm + cb) = cmw;
    *(unsigned*)(cv + cb) = cvw;
    if (lane_id() == 0) { am[b] = nm; av[b] = nv; }
}

static inline bool a8_grid_ok(int64_t nblk) { return (nblk + A8_WAVES - 1) / A8_WAVES <= 0x7fffffffLL; }

extern "C" int rv_adam8_quantize_f32(const float* x, int64_t n, uint8_t* codes, float* absmax, int kind, void* stream) {
    if (!x || !codes || !absmax || n <= 0 || (kind != 0 && kind != 1) || (((uintptr_t)x | (uintptr_t)absmax) & 3)) return RV_ERR_ARG;
    const int64_t nblk = (n + A8_BLOCK - 1) / A8_BLOCK;
    if (!a8_grid_ok(nblk)) return RV_ERR_ARG;
    hipLaunchKernelGGL(adam8_quantize_kernel, dim3(cdiv(nblk, A8_WAVES)), dim3(64 * A8_WAVES), 0, ST, x, (long)n, codes, absmax, kind, (long)nblk);
    return rv_check_launch();
}
extern "C" int rv_adam8_dequantize_f32(const uint8_t* codes, const float* absmax, int64_t n, int kind, float* x, void* stream) {
    if (!x || !codes || !absmax || n <= 0 || (kind != 0 && kind != 1) || (((uintptr_t)x | (uintptr_t)absmax) & 3)) return RV_ERR_ARG;
    const int64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(adam8_dequantize_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, ST, codes, absmax, (long)n, kind, x);
    return rv_check_launch();
}
extern "C" int rv_adamw8(void* p, float* master, const void* g, uint8_t* codes_m, uint8_t* codes_v, float* absmax_m, float* absmax_v,
                         const int64_t* table, int ntensors, int64_t nblocks, float lr, float b1, float b2, float eps, float wd, float bc1,
                         float bc2, const float* gscale, void* stream) {
    if (!p || !master || !g || !codes_m || !codes_v || !absmax_m || !absmax_v || !table || ntensors <= 0 || nblocks < ntensors) return RV_ERR_ARG;
    if ((((uintptr_t)p) | ((uintptr_t)g)) & 7) return RV_ERR_ARG;
    if (((uintptr_t)master) & 15) return RV_ERR_ARG;
    if ((((uintptr_t)codes_m) | ((uintptr_t)codes_v) | ((uintptr_t)absmax_m) | ((uintptr_t)absmax_v)) & 3) return RV_ERR_ARG;
    if (((uintptr_t)table) & 7) return RV_ERR_ARG;
    if (!a8_grid_ok(nblocks)) return RV_ERR_ARG;
    hipLaunchKernelGGL(adamw8_kernel, dim3(cdiv(nblocks, A8_WAVES)), dim3(64 * A8_WAVES), 0, ST, (bf16*)p, master, (const bf16*)g, codes_m, codes_v,
                       absmax_m, absmax_v, (const long*)table, ntensors, (long)nblocks, lr, b1, b2, eps, wd, bc1, bc2, gscale);
    return rv_check_launch();
}
