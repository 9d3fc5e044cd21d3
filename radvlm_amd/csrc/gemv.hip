// The skinny NT GEMM of decoding for gfx950, Y[M,N] = X[M,K] W[N,K]^T of one generated token per sequence (M = batch, 1..32 rows), in
// its three weight formats -- bf16, int8 rows (w8) and MXFP4 (w4) -- with the two row quantisers that write the packed copies, and the
// bf16 format with a live LoRA adapter (Y = X W^T + T_j B_j^T).  One split-K combine kernel and one host launch routine serve all four.
// Reductions use a fixed order that depends on the weight's shape only (N, K) -- never on M, on other rows or on timing -- and no
// atomics: a row's result is bit-identical whatever else shares its launch.  The quantised kernels rebuild in registers the bf16 weight
// W^ their quantiser left in place, with the bf16 kernel's K steps per wave, k-to-lane assignment per MFMA, ascending step order per
// accumulator, four-wave LDS reduction, combine and epilogue, so they are bit-identical to rv_gemv_bf16 on W^.
// Reference call sites are listed per entry point in include/radvlm_hip.h.
#include "common.h"
#include "radvlm_hip.h"

#include <type_traits>

namespace {

// ------------------------------------------------------------------------------------------------ skinny NT GEMM
// Y[M,N] = X[M,K] W[N,K]^T (+ bias) (+ residual), M <= 32.  Block: 4 waves, 64 output columns (four 16-column MFMA tiles); the K steps
// (32 deep) of the block's K range are split into 4 contiguous runs, one per wave.  Weights go straight from HBM to VGPRs (dwordx4, nt),
// U steps in flight per wave; the X rows (<= 64 KB, L2-resident) are loaded beside them.  MT = row tiles of 16 (rows >= M read zeros).
// MFMA 16x16x32: A = X rows (lane l: row l&15, k 8*(l>>4)..+7), B = W rows (lane l: column l&15, same k) -> D[row][col].
constexpr int GV_COLS = 64;
constexpr int GV_U = 4;

// W8: the weight operand is int8 with one fp32 scale per row (rv_quantize_rows_w8_bf16's packed rows) and the bf16 fragment
// bf16_rne(float(q) * s) is rebuilt in registers.  Same K steps per wave, same k-to-lane assignment per MFMA and every accumulator
// takes its steps in ascending order, so the result is bit-identical to the bf16 kernel on the dequantised weight.  Packed row:
// 64 bytes per PAIR of K steps; lane group kg's 16 bytes hold its 8 weights of step 2j, then its 8 of step 2j + 1 (one dwordx4 nt
// load feeds two MFMA steps); a trailing odd step and ragged K are zero-padded in the packed row.
// Step pairs in flight per wave.  2 (the bf16 kernel's four K steps per iteration at half its bytes) against 4 (its bytes in flight at twice
// the K per iteration) were both built and timed per decoder shape on one box (DESIGN.md 5b "8-bit decoder weights"; the records of both
// builds are in profiles/decode_ab_gemv.jsonl, mode w8, field `build`).  2 is the default: it needs fewer registers than the bf16 kernel
// (96 / 128 against 112 / 146, VGPR + AGPR), 4 needs 144 / 192 and leaves 3 / 2 waves per SIMD.  build.sh out.so -DRV_GV8_P=4 rebuilds
// the other.
#ifndef RV_GV8_P
#define RV_GV8_P 2
#endif
constexpr int GV8_P = RV_GV8_P;

DEVINL bf16x8 dq8(unsigned lo, unsigned hi, float s) {
    bf16x8 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        r[i] = f2bf((float)(int)(signed char)(lo >> (8 * i)) * s);
        r[4 + i] = f2bf((float)(int)(signed char)(hi >> (8 * i)) * s);
    }
    return r;
}

// The adapter of rv_gemv_lora_bf16, Y = X W^T + T_j B_j^T: after the bf16 K loop, wave 0 of slice 0 runs ceil(r / 32) more steps into the
// same accumulators with T in X's place (columns toff .. toff + r of T) and the block's rows of B_j in W's.  Every product of a zero B
// is a zero, so with B = 0 the accumulators, and every bit of Y, are rv_gemv_bf16's.  T and B are a few KB, read by every column block:
// plain loads, L2-resident.  A 64-column block lies in at most one module (boundaries are multiples of 64; the entry point checks), so
// the module is block-uniform.
constexpr int GV_MODS = 3;
struct GvLora {
    const bf16* T;
    long ldt;
    const bf16* b[GV_MODS];
    int c0[GV_MODS], c1[GV_MODS], toff[GV_MODS];
    int n_mod;
    long ldb;
    int r;
};

// What the weight operand needs beyond W and ldw is a trailing parameter pack: empty for bf16, the row scales (const float*) for int8,
// a GvLora for bf16 with a live adapter.  It is a pack, not a defaulted parameter, for one reason: the bf16 instantiation keeps the
// parent kernel's exact parameter list, and with it the parent's device code instruction for instruction (an extra pointer, or the bf16
// body moved into an inlined helper, changed its register allocation).  The adapter kind therefore adds its steps under `if constexpr`
// after the bf16 K loop, which it shares untouched; gemv_w4_kernel, whose parameter list differs, restates the prologue and epilogue.
template <typename... S> struct gv_kind { static constexpr bool w8 = false, lora = false; };
template <> struct gv_kind<const float*> { static constexpr bool w8 = true, lora = false; };
template <> struct gv_kind<GvLora> { static constexpr bool w8 = false, lora = true; };
template <typename A> DEVINL const A& gv_arg(const A& a) { return a; }

template <int MT, typename... S>
__global__ __launch_bounds__(256) void gemv_kernel(const bf16* __restrict__ X, long ldx, const bf16* __restrict__ W, long ldw, int M, int N,
                                                   int K, int split, float* __restrict__ part, void* __restrict__ Y, long ldy,
                                                   const bf16* __restrict__ bias, const bf16* __restrict__ R, long ldr, int out_f32,
                                                   S... kind_arg) {
    constexpr bool W8 = gv_kind<S...>::w8, LORA = gv_kind<S...>::lora;
    __shared__ float red[4][MT * 16][GV_COLS];
    const int lane = lane_id(), w = wave_id();
    const int c = lane & 15, kg = lane >> 4;
    const int n0 = blockIdx.x * GV_COLS;
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
        if constexpr (W8)                                           // packed rows of ldw bytes, 16 bytes per lane group and step pair
            wp[ct] = (const bf16*)((const char*)W + (long)(n_ok[ct] ? n : 0) * ldw + kg * 16);
        else
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
    if constexpr (W8) {
        const float* __restrict__ wscale = gv_arg(kind_arg...);
        float sc[4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) sc[ct] = n_ok[ct] ? wscale[n0 + ct * 16 + c] : 0.f;
        int st = s0;
        if ((st & 1) && st < s1) {                                  // the wave's range starts inside a pair: its second half alone
            const int k = st * 32;
            const bool kin = k + kg * 8 < K;
            u32x2 wq[4];
            bf16x8 xf[MT];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct)
                wq[ct] = (kin && n_ok[ct]) ? __builtin_nontemporal_load((const u32x2*)((const char*)wp[ct] + (long)(st >> 1) * 64 + 8))
                                           : u32x2{0u, 0u};
#pragma unroll
            for (int rt = 0; rt < MT; ++rt) xf[rt] = (kin && m_ok[rt]) ? *(const bf16x8*)(xp[rt] + k) : zero8();
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                const bf16x8 wf = dq8(wq[ct].x, wq[ct].y, sc[ct]);
#pragma unroll
                for (int rt = 0; rt < MT; ++rt) acc[rt][ct] = mfma16(xf[rt], wf, acc[rt][ct]);
            }
            ++st;
        }
        for (; st < s1; st += 2 * GV8_P) {
            u32x4 wq[GV8_P][4];
            bf16x8 xf[2 * GV8_P][MT];
#pragma unroll
            for (int p = 0; p < GV8_P; ++p) {
                const bool pin = st + 2 * p < s1;                   // a pair's 64 bytes exist whenever its first step does
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
                    wq[p][ct] = (pin && n_ok[ct])
                                    ? __builtin_nontemporal_load((const u32x4*)((const char*)wp[ct] + (long)((st >> 1) + p) * 64))
                                    : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int k = (st + 2 * p + h) * 32;
                    const bool kin = (st + 2 * p + h) < s1 && k + kg * 8 < K;
#pragma unroll
                    for (int rt = 0; rt < MT; ++rt) xf[2 * p + h][rt] = (kin && m_ok[rt]) ? *(const bf16x8*)(xp[rt] + k) : zero8();
                }
            }
#pragma unroll
            for (int p = 0; p < GV8_P; ++p) {
                const bool hin = st + 2 * p + 1 < s1;               // the pair's second step may belong to the next wave: zeros then
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    const bf16x8 w0 = dq8(wq[p][ct].x, wq[p][ct].y, sc[ct]);
#pragma unroll
                    for (int rt = 0; rt < MT; ++rt) acc[rt][ct] = mfma16(xf[2 * p][rt], w0, acc[rt][ct]);
                }
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    const bf16x8 w1 = dq8(hin ? wq[p][ct].z : 0u, hin ? wq[p][ct].w : 0u, sc[ct]);
#pragma unroll
                    for (int rt = 0; rt < MT; ++rt) acc[rt][ct] = mfma16(xf[2 * p + 1][rt], w1, acc[rt][ct]);
                }
            }
        }
    } else {
        for (int st = s0; st < s1; st += GV_U) {
            bf16x8 wf[GV_U][4], xf[GV_U][MT];
#pragma unroll
            for (int u = 0; u < GV_U; ++u) {
                const int k = (st + u) * 32;
                const bool kin = (st + u) < s1 && k + kg * 8 < K;       // K % 8 == 0: a lane's 8 elements are all in or all out
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) wf[u][ct] = (kin && n_ok[ct]) ? ld_nt(wp[ct] + k) : zero8();
#pragma unroll
                for (int rt = 0; rt < MT; ++rt) xf[u][rt] = (kin && m_ok[rt]) ? *(const bf16x8*)(xp[rt] + k) : zero8();
            }
#pragma unroll
            for (int u = 0; u < GV_U; ++u)
#pragma unroll
                for (int rt = 0; rt < MT; ++rt)
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = mfma16(xf[u][rt], wf[u][ct], acc[rt][ct]);
        }
    }
    if constexpr (LORA) {
        const GvLora& mods = gv_arg(kind_arg...);
        if (unit == 0) {                                                 // wave-uniform: the adapter's steps, after all of this wave's W steps
            int j = -1;
#pragma unroll
            for (int i = 0; i < GV_MODS; ++i)
                if (i < mods.n_mod && n0 >= mods.c0[i] && n0 < mods.c1[i]) j = i;
            if (j >= 0) {
                const bf16* __restrict__ Bj = j == 0 ? mods.b[0] : (j == 1 ? mods.b[1] : mods.b[2]);
                const int c0 = j == 0 ? mods.c0[0] : (j == 1 ? mods.c0[1] : mods.c0[2]);
                const int c1 = j == 0 ? mods.c1[0] : (j == 1 ? mods.c1[1] : mods.c1[2]);
                const int toff = j == 0 ? mods.toff[0] : (j == 1 ? mods.toff[1] : mods.toff[2]);
                for (int k = 0; k < mods.r; k += 32) {
                    const bool kin = k + kg * 8 < mods.r;                // r % 8 == 0
                    bf16x8 bfr[4], tf[MT];
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) {
                        const int n = n0 + ct * 16 + c;
                        bfr[ct] = (kin && n < c1) ? *(const bf16x8*)(Bj + (long)(n - c0) * mods.ldb + k + kg * 8) : zero8();
                    }
#pragma unroll
                    for (int rt = 0; rt < MT; ++rt)
                        tf[rt] = (kin && m_ok[rt]) ? *(const bf16x8*)(mods.T + (long)(rt * 16 + c) * mods.ldt + toff + k + kg * 8) : zero8();
#pragma unroll
                    for (int rt = 0; rt < MT; ++rt)
#pragma unroll
                        for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = mfma16(tf[rt], bfr[ct], acc[rt][ct]);
                }
            }
        }
    }
#pragma unroll
    for (int rt = 0; rt < MT; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[w][rt * 16 + 4 * kg + r][ct * 16 + c] = acc[rt][ct][r];
    __syncthreads();
    for (int idx = threadIdx.x; idx < MT * 16 * GV_COLS; idx += 256) {
        const int m = idx / GV_COLS, col = idx % GV_COLS, n = n0 + col;
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
        if (out_f32)
            ((float*)Y)[(long)m * ldy + n] = v;
        else
            ((bf16*)Y)[(long)m * ldy + n] = f2bf(v);
    }
}

// ------------------------------------------------------------------------------------------------ MXFP4 weights
// OCP Microscaling FP4: E2M1 elements, one E8M0 power-of-two scale per block of 32 consecutive k; a block is one 32-deep K step.  The
// quantised weight W^ = sign * value[code] * 2^e is a bf16 number by construction; rv_quantize_rows_mxfp4_bf16 writes it over the bf16
// weight and gemv_w4_kernel rebuilds the same bits in registers.  The rule is restated in numpy in tests/w4_ref.py.
// Packed row (private to the two kernels here, restated in w4_ref.pack_rows): 64 bytes per QUAD of K steps; lane group kg (k = 8 kg ..
// 8 kg + 7 of a step) owns bytes 16 kg .. 16 kg + 15 of a quad: 4 bytes per step u = 0..3, weight i of the group in bits 4 i .. 4 i + 3
// (nibble = sign << 3 | code).  One dwordx4 nontemporal load per lane feeds four MFMA steps.  The scale bytes (e + 127) are a separate
// uint8 [N][4 * quads] array, one dword per quad.  Padding past K: nibble 0, scale byte 127.
//
// Quads (four K steps, 64 bytes of a row) in flight per wave and iteration.  1 (four K steps, the bf16 kernel's GV_U, at a quarter of its
// bytes) against 2 were both built and timed per decoder shape on one box (DESIGN.md 5b "4-bit decoder weights"; the records of both
// builds are in profiles/decode_ab_gemv.jsonl, mode w4, field `build`).  1 is the default: equal or faster on the square and q|k|v shapes,
// within 3 % on the wide ones, and 64 / 82 VGPRs (M <= 16 / M <= 32) against 100 / 134.  build.sh out.so -DRV_GV4_Q=2 rebuilds the other.
#ifndef RV_GV4_Q
#define RV_GV4_Q 1
#endif
constexpr int GV4_Q = RV_GV4_Q;

// RV_W4_HWCVT = 1 (default): v_cvt_scalef32_pk_bf16_fp4, two nibbles and the block's scale 2^e to packed bf16 in one instruction.
// 0: the same bits by shifts and an exponent add (the result is the same by definition; DESIGN.md 5b records which one ships).
#ifndef RV_W4_HWCVT
#define RV_W4_HWCVT 1
#endif

// bf16 bits of sign * value[code] * 2^(sb - 127), value = {0, .5, 1, 1.5, 2, 3, 4, 6}: code >= 2 is E2M1's (exponent, mantissa) =
// (code >> 1, code & 1) with bias 1, so its bf16 exponent|mantissa field is (code << 6) + ((sb - 1) << 7); code 1 (E2M1's only
// subnormal, 0.5) is 2^(sb - 128) with mantissa 0.  sb >= 5 by the rule, so every nonzero result is a normal bf16 number.
DEVINL unsigned w4_bits(unsigned nib, unsigned sb) {
    const unsigned c = nib & 7u;
    const unsigned t = (c == 1u ? 0u : c << 6) + ((sb - 1u) << 7);
    return c ? (t | (nib & 8u) << 12) : 0u;
}

// the 8 weights of one lane group and step (one dword of nibbles) at scale byte sb
DEVINL bf16x8 dq4(unsigned q, unsigned sb) {
    bf16x8 r;
#if RV_W4_HWCVT
    const float s = __uint_as_float(sb << 23);
    const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, s, 0), b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, s, 1),
                 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, s, 2), d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, s, 3);
    r[0] = a[0]; r[1] = a[1]; r[2] = b[0]; r[3] = b[1]; r[4] = c[0]; r[5] = c[1]; r[6] = d[0]; r[7] = d[1];
#else
    typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;
    u16x8 v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (unsigned short)w4_bits(q >> (4 * i), sb);
    r = __builtin_bit_cast(bf16x8, v);
#endif
    return r;
}

// Y[M,N] = X[M,K] W^[N,K]^T (+ bias) (+ residual), M <= 32: gemv_kernel above with the weight fragment rebuilt from nibbles.
// A wave's step range [s0, s1) may start at any step index mod 4 and may be empty: up to three head steps are read as single dwords,
// then whole quads; steps of a quad at or past s1 (the next wave's, or padding) meet x = 0, as the bf16 kernel's masked steps do.
template <int MT>
__global__ __launch_bounds__(256) void gemv_w4_kernel(const bf16* __restrict__ X, long ldx, const unsigned char* __restrict__ P, long ldp,
                                                      const unsigned char* __restrict__ S, long lds, int M, int N, int K, int split,
                                                      float* __restrict__ part, void* __restrict__ Y, long ldy, const bf16* __restrict__ bias,
                                                      const bf16* __restrict__ R, long ldr, int out_f32) {
    __shared__ float red[4][MT * 16][GV_COLS];
    const int lane = lane_id(), w = wave_id();
    const int c = lane & 15, kg = lane >> 4;
    const int n0 = blockIdx.x * GV_COLS;
    const int sidx = blockIdx.y;
    const int ks = (K + 31) / 32;
    const int unit = sidx * 4 + w, units = split * 4;
    const int s0 = (int)((long)ks * unit / units), s1 = (int)((long)ks * (unit + 1) / units);
    const unsigned char* wp[4];
    const unsigned char* sp[4];
    bool n_ok[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        const int n = n0 + ct * 16 + c;
        n_ok[ct] = n < N;
        wp[ct] = P + (long)(n_ok[ct] ? n : 0) * ldp + kg * 16;
        sp[ct] = S + (long)(n_ok[ct] ? n : 0) * lds;
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
    int st = s0;
    if ((st & 3) && st < s1) {                                      // the wave's range starts inside a quad: its steps up to the quad's end
        const int h1 = min(s1, (st + 3) & ~3);
        unsigned wq[3][4], sb[4];
        bf16x8 xf[3][MT];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) sb[ct] = *(const unsigned*)(sp[ct] + (long)(st >> 2) * 4);
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int step = st + u, k = step * 32;
            const bool in = step < h1, kin = in && k + kg * 8 < K;
#pragma unroll
            for (int ct = 0; ct < 4; ++ct)
                wq[u][ct] = (in && n_ok[ct]) ? __builtin_nontemporal_load((const unsigned*)(wp[ct] + (long)(st >> 2) * 64 + (step & 3) * 4)) : 0u;
#pragma unroll
            for (int rt = 0; rt < MT; ++rt) xf[u][rt] = (kin && m_ok[rt]) ? *(const bf16x8*)(xp[rt] + k) : zero8();
        }
#pragma unroll
        for (int u = 0; u < 3; ++u)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                const bf16x8 wf = dq4(wq[u][ct], (sb[ct] >> (8 * ((st + u) & 3))) & 0xffu);
#pragma unroll
                for (int rt = 0; rt < MT; ++rt) acc[rt][ct] = mfma16(xf[u][rt], wf, acc[rt][ct]);
            }
        st = h1;
    }
    for (; st < s1; st += 4 * GV4_Q) {
        u32x4 wq[GV4_Q][4];
        unsigned sb[GV4_Q][4];
        bf16x8 xf[4 * GV4_Q][MT];
#pragma unroll
        for (int q = 0; q < GV4_Q; ++q) {
            const bool qin = st + 4 * q < s1;                       // a quad's 64 bytes and 4 scale bytes exist whenever its first step does
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                wq[q][ct] = (qin && n_ok[ct]) ? __builtin_nontemporal_load((const u32x4*)(wp[ct] + (long)((st >> 2) + q) * 64))
                                              : u32x4{0u, 0u, 0u, 0u};
                sb[q][ct] = qin ? *(const unsigned*)(sp[ct] + (long)((st >> 2) + q) * 4) : 0x7f7f7f7fu;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = (st + 4 * q + u) * 32;
                const bool kin = (st + 4 * q + u) < s1 && k + kg * 8 < K;
#pragma unroll
                for (int rt = 0; rt < MT; ++rt) xf[4 * q + u][rt] = (kin && m_ok[rt]) ? *(const bf16x8*)(xp[rt] + k) : zero8();
            }
        }
#pragma unroll
        for (int q = 0; q < GV4_Q; ++q)
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    const bf16x8 wf = dq4(wq[q][ct][u], (sb[q][ct] >> (8 * u)) & 0xffu);
#pragma unroll
                    for (int rt = 0; rt < MT; ++rt) acc[rt][ct] = mfma16(xf[4 * q + u][rt], wf, acc[rt][ct]);
                }
    }
#pragma unroll
    for (int rt = 0; rt < MT; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[w][rt * 16 + 4 * kg + r][ct * 16 + c] = acc[rt][ct][r];
    __syncthreads();
    for (int idx = threadIdx.x; idx < MT * 16 * GV_COLS; idx += 256) {
        const int m = idx / GV_COLS, col = idx % GV_COLS, n = n0 + col;
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
        if (out_f32)
            ((float*)Y)[(long)m * ldy + n] = v;
        else
            ((bf16*)Y)[(long)m * ldy + n] = f2bf(v);
    }
}

// split-K combine: the K-slices summed in slice order, then bias / residual / store (same epilogue as above)
__global__ void gemv_combine_kernel(const float* __restrict__ part, int split, int M, int N, void* __restrict__ Y, long ldy,
                                    const bf16* __restrict__ bias, const bf16* __restrict__ R, long ldr, int out_f32) {
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= (long)M * N) return;
    const int m = (int)(tid / N), n = (int)(tid % N);
    float v = part[tid];
    for (int s = 1; s < split; ++s) v += part[(long)s * M * N + tid];
    if (bias) v += bf2f(bias[n]);
    if (R) v += bf2f(R[(long)m * ldr + n]);
    if (out_f32)
        ((float*)Y)[(long)m * ldy + n] = v;
    else
        ((bf16*)Y)[(long)m * ldy + n] = f2bf(v);
}

// ------------------------------------------------------------------------------------------------ int8 row quantisation
// One workgroup per weight row: absmax, s = amax / 127 (1 for a zero row), q = clamp(rint(w / s)), W <- bf16_rne(float(q) * s) in place,
// q into the packed row gemv_kernel's int8 instantiation reads.  IEEE division and rint (round half to even); max is order-free, no
// atomics.  The in-place write is race-free because (a) every load of pass 1 is consumed before the __syncthreads() after the wave
// reduction, which all threads pass before any thread writes, and (b) in pass 2 the map g -> k is a bijection onto the row's 8-element
// groups, so each group is read and written by one thread only (not the thread that read it in pass 1: the barrier orders those).
__global__ __launch_bounds__(256) void quantize_rows_w8_kernel(bf16* __restrict__ W, long ldw, signed char* __restrict__ Q, long ldq,
                                                               float* __restrict__ scale, int K) {
    __shared__ float red[4];
    bf16* row = W + (long)blockIdx.x * ldw;
    signed char* qrow = Q + (long)blockIdx.x * ldq;
    float amax = 0.f;
    for (int k = threadIdx.x * 8; k < K; k += 256 * 8) {
        const bf16x8 t = *(const bf16x8*)(row + k);
#pragma unroll
        for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(bf2f(t[i])));
    }
    amax = wave_max(amax);
    if (lane_id() == 0) red[wave_id()] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float s = amax > 0.f ? amax / 127.f : 1.f;
    if (threadIdx.x == 0) scale[blockIdx.x] = s;
    // packed group g (8 bytes): pair g / 8, lane group (g % 8) / 2, half g % 2 -> k = (2 * pair + half) * 32 + 8 * group
    for (int g = threadIdx.x; g < ldq / 8; g += 256) {
        const int k = (2 * (g >> 3) + (g & 1)) * 32 + ((g & 7) >> 1) * 8;
        unsigned lo = 0u, hi = 0u;
        if (k < K) {
            const bf16x8 t = *(const bf16x8*)(row + k);
            bf16x8 o;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float q = fminf(fmaxf(rintf(bf2f(t[i]) / s), -127.f), 127.f);
                o[i] = f2bf(q * s);
                const unsigned b = (unsigned)(int)q & 0xffu;
                if (i < 4) lo |= b << (8 * i);
                else hi |= b << (8 * (i - 4));
            }
            *(bf16x8*)(row + k) = o;
        }
        *(u32x2*)(qrow + (long)g * 8) = u32x2{lo, hi};
    }
}

// ------------------------------------------------------------------------------------------------ MXFP4 row quantisation
// One workgroup per weight row, one thread per block of 32 (a K step): amax over the block's existing entries, e = exponent(amax) - 2
// (0 for an all-zero block), a = |w| 2^-e (exact), code = nearest of {0, .5, 1, 1.5, 2, 3, 4, 6} with ties to the even code (a > 6
// saturates to 7), W <- sign * value[code] * 2^e in place (+0.0 for code 0), nibbles and scale byte into the packed rows.  Steps past K
// up to the quad's end get nibble 0 and scale byte 127.  A thread reads and writes its own block only: no barrier, no atomics.
__global__ __launch_bounds__(256) void quantize_rows_mxfp4_kernel(bf16* __restrict__ W, long ldw, unsigned char* __restrict__ P, long ldp,
                                                                  unsigned char* __restrict__ S, long lds, int K) {
    bf16* row = W + (long)blockIdx.x * ldw;
    unsigned char* prow = P + (long)blockIdx.x * ldp;
    unsigned char* srow = S + (long)blockIdx.x * lds;
    for (int step = threadIdx.x; step < (int)lds; step += 256) {
        const int k0 = step * 32;
        bf16x8 t[4];
        float amax = 0.f;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            t[g] = k0 + g * 8 < K ? *(const bf16x8*)(row + k0 + g * 8) : zero8();       // K % 8 == 0: a group is all in or all out
#pragma unroll
            for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(bf2f(t[g][i])));
        }
        const unsigned sb = amax > 0.f ? ((__float_as_uint(amax) >> 23) & 0xffu) - 2u : 127u;
        const float inv = __uint_as_float((254u - sb) << 23);                               // 2^-e
        srow[step] = (unsigned char)sb;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            unsigned q = 0u;
            typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;
            u16x8 o;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float wv = bf2f(t[g][i]);
                const float a = fabsf(wv) * inv;
                const unsigned code = (unsigned)(a > 0.25f) + (unsigned)(a >= 0.75f) + (unsigned)(a > 1.25f) + (unsigned)(a >= 1.75f) +
                                      (unsigned)(a > 2.5f) + (unsigned)(a >= 3.5f) + (unsigned)(a > 5.f);
                const unsigned nib = code ? (code | (wv < 0.f ? 8u : 0u)) : 0u;
                q |= nib << (4 * i);
                o[i] = (unsigned short)w4_bits(nib, sb);
            }
            if (k0 + g * 8 < K) *(bf16x8*)(row + k0 + g * 8) = __builtin_bit_cast(bf16x8, o);
            *(unsigned*)(prow + (long)(step >> 2) * 64 + g * 16 + (step & 3) * 4) = q;
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
// The one launch routine behind the four rv_gemv_* entry points: the checks every format shares, the K split and its workspace, the
// grid, the row-tile count MT, the combine.  An entry point passes whether its own weight operand is acceptable and
// launch(MT as an integral_constant, grid, split, part), which starts its kernel: the kernels' parameter lists differ.
template <typename Launch>
int gemv_launch(bool w_ok, const void* X, int64_t ldx, void* Y, int64_t ldy, const void* bias, const void* residual, int64_t ldr, int M,
                int N, int K, int out_f32, void* workspace, int64_t ws_bytes, void* stream, Launch launch) {
    if (!w_ok || !X || !Y || M < 1 || M > 32 || N <= 0 || K <= 0 || (K & 7) || (ldx & 7) || ldx < K || ldy < N || (residual && ldr < N))
        return RV_ERR_ARG;
    const int split = rv_gemv_split(N, K);
    float* part = nullptr;
    if (split > 1) {
        if (!workspace || ws_bytes < (int64_t)split * M * N * 4) return RV_ERR_ARG;
        part = (float*)workspace;
    }
    const dim3 grid(cdiv(N, GV_COLS), split);
    if (M <= 16)
        launch(std::integral_constant<int, 1>(), grid, split, part);
    else
        launch(std::integral_constant<int, 2>(), grid, split, part);
    if (split > 1)
        hipLaunchKernelGGL(gemv_combine_kernel, dim3(cdiv((long)M * N, 256)), dim3(256), 0, ST, (const float*)part, split, M, N, Y, (long)ldy,
                           (const bf16*)bias, (const bf16*)residual, (long)ldr, out_f32);
    return rv_check_launch();
}

}  // namespace

extern "C" int rv_gemv_split(int N, int K) {
    // K slices per column block: enough blocks for >= 2 per CU on 256 CUs, every wave keeps >= 2 of its 32-deep K steps.  A function of
    // (N, K) only, so a row's reduction order never depends on M.
    const long nb = (N + GV_COLS - 1) / GV_COLS, ks = (K + 31) / 32;
    int split = 1;
    while (nb * split < 512 && split < 16 && ks >= (long)split * 2 * 4 * 2) split *= 2;
    return split;
}

extern "C" int rv_gemv_bf16(const void* X, int64_t ldx, const void* W, int64_t ldw, void* Y, int64_t ldy, const void* bias, const void* residual,
                            int64_t ldr, int M, int N, int K, int out_f32, void* workspace, int64_t ws_bytes, void* stream) {
    return gemv_launch(W && !(ldw & 7) && ldw >= K, X, ldx, Y, ldy, bias, residual, ldr, M, N, K, out_f32, workspace, ws_bytes, stream,
                       [&](auto mt, dim3 grid, int split, float* part) {
                           hipLaunchKernelGGL(gemv_kernel<mt()>, grid, dim3(256), 0, ST, (const bf16*)X, (long)ldx, (const bf16*)W, (long)ldw, M, N,
                                              K, split, part, Y, (long)ldy, (const bf16*)bias, (const bf16*)residual, (long)ldr, out_f32);
                       });
}

extern "C" int rv_gemv_lora_bf16(const void* X, int64_t ldx, const void* W, int64_t ldw, const void* T, int64_t ldt, int r, int n_mod,
                                 const void* B0, int col0_0, int col1_0, int toff0, const void* B1, int col0_1, int col1_1, int toff1, const void* B2,
                                 int col0_2, int col1_2, int toff2, int64_t ldb, void* Y, int64_t ldy, const void* bias, const void* residual,
                                 int64_t ldr, int M, int N, int K, void* workspace, int64_t ws_bytes, void* stream) {
    // its own checks: the rank, T / B alignment and strides, then the module table; gemv_launch makes the rest
    if (!T || !lora_rank_ok(r) || n_mod < 1 || n_mod > GV_MODS || (ldt & 7) || (ldb & 7) || ldb < r || !aligned16(X) || !aligned16(W) ||
        !aligned16(T))
        return RV_ERR_ARG;
    const void* b[GV_MODS] = {B0, B1, B2};
    const int c0[GV_MODS] = {col0_0, col0_1, col0_2}, c1[GV_MODS] = {col1_0, col1_1, col1_2}, to[GV_MODS] = {toff0, toff1, toff2};
    GvLora mods;
    mods.T = (const bf16*)T, mods.ldt = (long)ldt, mods.n_mod = n_mod, mods.ldb = (long)ldb, mods.r = r;
    int prev = 0;
    for (int j = 0; j < GV_MODS; ++j) {
        if (j < n_mod) {
            // ascending, disjoint column ranges; a boundary inside Y is a multiple of 64 (a column block never straddles two modules)
            if (!b[j] || !aligned16(b[j]) || c0[j] < prev || c1[j] <= c0[j] || c1[j] > N || (c0[j] % GV_COLS) || (c1[j] != N && (c1[j] % GV_COLS)) ||
                to[j] < 0 || (to[j] & 7) || (int64_t)to[j] + r > ldt)
                return RV_ERR_ARG;
            prev = c1[j];
        }
        mods.b[j] = (const bf16*)(j < n_mod ? b[j] : b[0]);
        mods.c0[j] = j < n_mod ? c0[j] : 0;
        mods.c1[j] = j < n_mod ? c1[j] : 0;
        mods.toff[j] = j < n_mod ? to[j] : 0;
    }
    return gemv_launch(W && !(ldw & 7) && ldw >= K, X, ldx, Y, ldy, bias, residual, ldr, M, N, K, 0, workspace, ws_bytes, stream,
                       [&](auto mt, dim3 grid, int split, float* part) {
                           hipLaunchKernelGGL((gemv_kernel<mt(), GvLora>), grid, dim3(256), 0, ST, (const bf16*)X, (long)ldx, (const bf16*)W,
                                              (long)ldw, M, N, K, split, part, Y, (long)ldy, (const bf16*)bias, (const bf16*)residual, (long)ldr,
                                              0, mods);
                       });
}

extern "C" int64_t rv_w8_row_bytes(int K) { return (((int64_t)K + 31) / 32 + 1) / 2 * 64; }

extern "C" int rv_quantize_rows_w8_bf16(void* W, int64_t ldw, void* packed, int64_t ldp, float* scale, int N, int K, void* stream) {
    if (!W || !packed || !scale || N <= 0 || K <= 0 || (K & 7) || (ldw & 7) || ldw < K || ldp != rv_w8_row_bytes(K)) return RV_ERR_ARG;
    hipLaunchKernelGGL(quantize_rows_w8_kernel, dim3(N), dim3(256), 0, ST, (bf16*)W, (long)ldw, (signed char*)packed, (long)ldp, scale, K);
    return rv_check_launch();
}

extern "C" int rv_gemv_w8_bf16(const void* X, int64_t ldx, const void* packed, int64_t ldp, const float* scale, void* Y, int64_t ldy,
                               const void* bias, const void* residual, int64_t ldr, int M, int N, int K, int out_f32, void* workspace,
                               int64_t ws_bytes, void* stream) {
    return gemv_launch(packed && scale && ldp == rv_w8_row_bytes(K), X, ldx, Y, ldy, bias, residual, ldr, M, N, K, out_f32, workspace, ws_bytes,
                       stream, [&](auto mt, dim3 grid, int split, float* part) {
                           hipLaunchKernelGGL((gemv_kernel<mt(), const float*>), grid, dim3(256), 0, ST, (const bf16*)X, (long)ldx,
                                              (const bf16*)packed, (long)ldp, M, N, K, split, part, Y, (long)ldy, (const bf16*)bias,
                                              (const bf16*)residual, (long)ldr, out_f32, scale);
                       });
}

extern "C" int64_t rv_w4_row_bytes(int K) { return (((int64_t)K + 31) / 32 + 3) / 4 * 64; }

extern "C" int64_t rv_w4_scale_row_bytes(int K) { return (((int64_t)K + 31) / 32 + 3) / 4 * 4; }

extern "C" int rv_quantize_rows_mxfp4_bf16(void* W, int64_t ldw, void* packed, int64_t ldp, void* scales, int64_t lds, int N, int K,
                                           void* stream) {
    if (!W || !packed || !scales || N <= 0 || K <= 0 || (K & 7) || (ldw & 7) || ldw < K || ldp != rv_w4_row_bytes(K) ||
        lds != rv_w4_scale_row_bytes(K))
        return RV_ERR_ARG;
    hipLaunchKernelGGL(quantize_rows_mxfp4_kernel, dim3(N), dim3(256), 0, ST, (bf16*)W, (long)ldw, (unsigned char*)packed, (long)ldp,
                       (unsigned char*)scales, (long)lds, K);
    return rv_check_launch();
}

extern "C" int rv_gemv_w4_bf16(const void* X, int64_t ldx, const void* packed, int64_t ldp, const void* scales, int64_t lds, void* Y,
                               int64_t ldy, const void* bias, const void* residual, int64_t ldr, int M, int N, int K, int out_f32,
                               void* workspace, int64_t ws_bytes, void* stream) {
    return gemv_launch(packed && scales && ldp == rv_w4_row_bytes(K) && lds == rv_w4_scale_row_bytes(K), X, ldx, Y, ldy, bias, residual, ldr, M,
                       N, K, out_f32, workspace, ws_bytes, stream, [&](auto mt, dim3 grid, int split, float* part) {
                           hipLaunchKernelGGL(gemv_w4_kernel<mt()>, grid, dim3(256), 0, ST, (const bf16*)X, (long)ldx,
                                              (const unsigned char*)packed, (long)ldp, (const unsigned char*)scales, (long)lds, M, N, K, split,
                                              part, Y, (long)ldy, (const bf16*)bias, (const bf16*)residual, (long)ldr, out_f32);
                       });
}
