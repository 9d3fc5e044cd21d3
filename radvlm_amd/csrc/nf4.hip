// NF4 frozen decoder base of a LoRA run (QLoRA, --bits 4 --quant_type nf4): 64 weights per block counted from a tensor's first element, one
// fp32 absmax per block, sixteen fp32 levels (nf4_codebook.h), two codes per byte (element 2j in the high nibble).  With double
// quantisation the absmax of a block is rebuilt from one code byte of the signed 8-bit table (adam8_codebook.h), one fp32 scale per 256
// blocks and one fp32 offset per tensor.  The rule is stated in tests/nf4_ref.py; these kernels are held to it bit for bit.
//   rv_nf4_quantize_bf16  the one-time act at load: one wave per block, one element per lane, the maximum by wave shuffles (order-free)
//   rv_nf4_dequant_bf16   the hot kernel: one launch writes every tensor of a table (a decoder layer's seven matrices) into the bf16
//                         scratch that the unchanged GEMMs read.  Pure streaming: 0.5 B read and 2 B written per weight, no atomics.
#include "common.h"
#define RV_NF4_TABLE __device__ const
#include "nf4_codebook.h"
#define RV_ADAM8_TABLE __device__ const
#include "adam8_codebook.h"
#include "radvlm_hip.h"

#define NF4_BLOCK 64
#define NF4_WAVES 4
#define NF4_LANE 8                              // weights per lane and step: one 4-byte code load, one 16-byte bf16 store
#define NF4_STEPS 4
#define NF4_CHUNK (64 * NF4_LANE * NF4_STEPS)   // weights per wave: 2048 = 32 blocks; a chunk never straddles two tensors

// The level of a code: a read of the 16-entry LDS table (64 lanes, at most 16 distinct banks: conflict-free).  Measured against it and
// not kept: the levels as a four-level select tree on literals (no LDS read, 15 v_cndmask per weight: 1.5x slower), and
// nontemporal code loads (inside the spread).
DEVINL float nf4_level(const float* t, unsigned c) { return t[c]; }
DEVINL unsigned nf4_ld4(const uint8_t* p) { return *(const unsigned*)p; }

// ------------------------------------------------------------------------------------------------ quantise one tensor
__global__ __launch_bounds__(64 * NF4_WAVES) void nf4_quantize_kernel(const bf16* x, long n, uint8_t* codes, float* absmax, long nblk) {
    __shared__ float mid[16];                   // mid[i] = fp32((float64(t[i]) + float64(t[i + 1])) / 2): the sum is exact, one rounding
    if (threadIdx.x < 15)
        mid[threadIdx.x] = (float)(((double)__uint_as_float(rv_nf4_bits[threadIdx.x]) + (double)__uint_as_float(rv_nf4_bits[threadIdx.x + 1])) * 0.5);
    __syncthreads();
    const long b = (long)blockIdx.x * NF4_WAVES + wave_id();
    if (b >= nblk) return;
    const long e = b * NF4_BLOCK + lane_id();
    const float xv = e < n ? bf2f(x[e]) : 0.f;
    const float am = wave_max(fabsf(xv));
    const float a = xv / (am != 0.f ? am : 1.f);
    int c = 0;                                  // the number of midpoints strictly below a: four halvings over the 15 sorted midpoints
#pragma unroll
    for (int s = 8; s > 0; s >>= 1) c += mid[c + s - 1] < a ? s : 0;
    const int next = __shfl_down(c, 1, 64);     // the odd element of the byte (every lane takes part in the shuffle)
    if (e < n && !(lane_id() & 1)) codes[e >> 1] = (uint8_t)((c << 4) | (e + 1 < n ? next : 0));
    if (lane_id() == 0) absmax[b] = am;
}

// ------------------------------------------------------------------------------------------------ dequantise a table of tensors
// tab: int64 [6, T] = first chunk (0 for the first; tensor t owns ceil(length / 2048) consecutive chunks), first code byte, first absmax
// entry, length (> 0), first destination element, first second-level scale.  Chunk c belongs to the tensor found by a wave-uniform
// search.  A chunk that is full, whose code bytes are 4-byte aligned and whose destination is 16-byte aligned takes the vector form
// (the four code loads first, then the arithmetic and the stores); any other takes byte loads and 2-byte stores, masked past the end.
template <bool DQ>
DEVINL float nf4_absmax(const float* absmax, const uint8_t* acodes, const float* scale2, const float* q8, long am0, long s20, float off, long blk) {
    if (!DQ) return absmax[am0 + blk];
    return __fadd_rn(__fmul_rn(q8[acodes[am0 + blk]], scale2[s20 + (blk >> 8)]), off);
}
template <bool DQ>
__global__ __launch_bounds__(64 * NF4_WAVES) void nf4_dequant_kernel(const uint8_t* codes, const float* absmax, const uint8_t* acodes, const float* scale2,
                                                                     const float* offset, const long* tab, int T, long nchunks, bf16* dst) {
    __shared__ float t[16];
    __shared__ float q8[DQ ? 256 : 1];
    if (threadIdx.x < 16) t[threadIdx.x] = __uint_as_float(rv_nf4_bits[threadIdx.x]);
    if (DQ) q8[threadIdx.x] = __uint_as_float(rv_adam8_signed_bits[threadIdx.x]);          // 256 threads, 256 entries
    __syncthreads();
    const long c = (long)blockIdx.x * NF4_WAVES + wave_id();
    if (c >= nchunks) return;
    int lo = 0, hi = T;                                      // wave-uniform: the last tensor whose first chunk is <= c
    while (hi - lo > 1) {
        const int m = (lo + hi) >> 1;
        if (tab[m] <= c) lo = m; else hi = m;
    }
    const long n = tab[3 * (long)T + lo], am0 = tab[2 * (long)T + lo], s20 = tab[5 * (long)T + lo];
    const uint8_t* cp = codes + tab[(long)T + lo];
    bf16* out = dst + tab[4 * (long)T + lo];
    const float off = DQ ? offset[lo] : 0.f;
    const long e0 = (c - tab[lo]) * NF4_CHUNK + lane_id() * NF4_LANE;
    const bool vec = (c - tab[lo] + 1) * NF4_CHUNK <= n && !((uintptr_t)cp & 3) && !((uintptr_t)out & 15);
    if (vec) {
        unsigned w[NF4_STEPS];
        float am[NF4_STEPS];
#pragma unroll
        for (int s = 0; s < NF4_STEPS; ++s) {
            const long e = e0 + s * 64 * NF4_LANE;
            w[s] = nf4_ld4(cp + (e >> 1));
            am[s] = nf4_absmax<DQ>(absmax, acodes, scale2, q8, am0, s20, off, e >> 6);
        }
#pragma unroll
        for (int s = 0; s < NF4_STEPS; ++s) {
            bf16x8 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) {                    // byte k of the little-endian word: elements 2k (high nibble) and 2k + 1 (low)
                const unsigned byte = (w[s] >> (8 * k)) & 255u;
                o[2 * k] = f2bf(__fmul_rn(nf4_level(t, byte >> 4), am[s]));
                o[2 * k + 1] = f2bf(__fmul_rn(nf4_level(t, byte & 15u), am[s]));
            }
            *(bf16x8*)(out + e0 + s * 64 * NF4_LANE) = o;
        }
        return;
    }
    for (int s = 0; s < NF4_STEPS; ++s) {
        const long e = e0 + s * 64 * NF4_LANE;
        if (e >= n) break;
        const float am = nf4_absmax<DQ>(absmax, acodes, scale2, q8, am0, s20, off, e >> 6);      // 8 | 64: the lane's elements share a block
        for (int j = 0; j < NF4_LANE && e + j < n; ++j) {
            const unsigned byte = cp[(e + j) >> 1];
            out[e + j] = f2bf(__fmul_rn(nf4_level(t, (j & 1) ? (byte & 15u) : (byte >> 4)), am));
        }
    }
}

extern "C" int rv_nf4_quantize_bf16(const void* x, int64_t n, uint8_t* codes, float* absmax, void* stream) {
    if (!x || !codes || !absmax || n <= 0 || ((uintptr_t)x & 1) || ((uintptr_t)absmax & 3)) return RV_ERR_ARG;
    const int64_t nblk = (n + NF4_BLOCK - 1) / NF4_BLOCK;
    if ((nblk + NF4_WAVES - 1) / NF4_WAVES > 0x7fffffffLL) return RV_ERR_ARG;
    hipLaunchKernelGGL(nf4_quantize_kernel, dim3(cdiv(nblk, NF4_WAVES)), dim3(64 * NF4_WAVES), 0, ST, (const bf16*)x, (long)n, codes, absmax, (long)nblk);
    return rv_check_launch();
}
extern "C" int rv_nf4_dequant_bf16(const uint8_t* codes, const float* absmax, const uint8_t* absmax_codes, const float* scale2, const float* offset,
                                   const int64_t* table, int ntensors, int64_t nchunks, void* dst, void* stream) {
    if (!codes || !table || !dst || ntensors <= 0 || nchunks < ntensors || ((uintptr_t)table & 7) || ((uintptr_t)dst & 1)) return RV_ERR_ARG;
    const bool dq = absmax == nullptr;
    if (dq ? (!absmax_codes || !scale2 || !offset || (((uintptr_t)scale2 | (uintptr_t)offset) & 3)) : ((uintptr_t)absmax & 3) != 0) return RV_ERR_ARG;
    if ((nchunks + NF4_WAVES - 1) / NF4_WAVES > 0x7fffffffLL) return RV_ERR_ARG;
    const dim3 grid(cdiv(nchunks, NF4_WAVES)), block(64 * NF4_WAVES);
    if (dq)
        hipLaunchKernelGGL(nf4_dequant_kernel<true>, grid, block, 0, ST, codes, absmax, absmax_codes, scale2, offset, (const long*)table, ntensors,
                           (long)nchunks, (bf16*)dst);
    else
        hipLaunchKernelGGL(nf4_dequant_kernel<false>, grid, block, 0, ST, codes, absmax, absmax_codes, scale2, offset, (const long*)table, ntensors,
                           (long)nchunks, (bf16*)dst);
    return rv_check_launch();
}
