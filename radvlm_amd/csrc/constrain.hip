// Constrained decoding for gfx950: the kernel that restricts a decode step's raw fp32 logits rows to the tokens a deterministic
// automaton over token ids allows (generate(constraint=), radvlm_amd/constraints.py), in place.  The automaton is in CSR form: state s
// allows the ids edge_tok[edge_off[s] .. edge_off[s + 1]), strictly ascending, and taking id edge_tok[e] leads to edge_next[e].  A row's
// state is live (s >= 0), free (-1: the row is not accessed; where an EOS edge leads, and what an unconstrained row carries) or dead
// (-2, and every other value outside [0, n_states): the whole row becomes -inf).
//
// Per row r, with si = slot ? slot[r] : r and s = state[si]:
//   advance  (tok != NULL; tok[r] is the token chosen from this row's previous step)  a live s becomes the edge_next of the edge
//            (s, tok[r]), or -2 when s has no such edge; a negative s stays; the new s is written back to state[si].
//   mask     s == -1: nothing.  Dead: columns [0, n) <- -inf.  Live: every column of [0, n) that is not an allowed id <- -inf; the
//            allowed columns are neither read nor written, so their bits stay (NaN payloads and -0.0 included).
// The kernel loads no logit at all: it only stores.  Columns >= n of an ld-wide row are never written.  Edge ids outside [0, n) are
// ignored.
//
// Relation to HF: PrefixConstrainedLogitsProcessor adds a mask of 0 / -inf after MinNewTokensLength and before SuppressTokens.  Every
// processor of rv_logits_process_argmax*_f32 other than the repetition penalty only writes -inf, and the penalty maps -inf to -inf
// (-inf * p = -inf / p = -inf for p > 0), so masking first and running the fused kernel unchanged gives HF's row.  Two differences:
// an allowed -0.0 keeps its sign (HF's `+ 0.0` makes it +0.0), and a banned NaN / +inf becomes -inf where HF's `+ -inf` keeps NaN for
// the NaN (the deviation the bad-words processor already documents).
//
// Launch structure: one workgroup of 256 per row, one launch for advance and mask.  The advance writes state[si] and the mask reads it,
// so the two stay inside one workgroup: cutting a row over several workgroups would let one of them read a state another has already
// advanced.  The edge of (s, tok) is found by a 256-ary search (each round, thread t probes the t-th of 256 pieces and the last probe
// <= tok wins through an LDS maximum): at most three rounds for 2^24 edges, where a binary search by one thread is 18 dependent loads
// for a state that allows a whole 152,064-id vocabulary.  The mask keeps one bit per column of the whole row in LDS (262,144 bits =
// 32 KiB): the words of [0, n) are cleared, the threads read the state's edge run with lanes on consecutive edges and set the bits of
// its ids (LDS atomic or; the run is sorted, so a thread stops at the first id >= n), and then the row is swept once: four columns
// per thread and step, one 16-byte store where all four are banned and the row is 16-byte aligned, single stores elsewhere.  A first
// version swept the row in tiles of 4,096 columns with a bitmap per tile; every tile then waited for its own dependent load of the
// edge run and handed the next tile its first edge through an LDS maximum that all 256 threads hit, and a state that allows every
// id took 1.25 ms at 152,064 columns (DESIGN.md 5b "Constrained decoding" has both measurements).  LDS atomics only; nothing global is
// read-modified.  Rows are independent: a row's bits and its new state depend on that row's state, token and edge run alone, not on
// `rows` or the other rows.
//
// Tables the host did not validate cannot fault: a run's bounds are clamped into [0, n_edges], an id outside [0, n) sets no bit, a
// slot outside [0, state_rows) makes the row dead and writes no state.  Two rows of one launch must not name the same slot.
#include "common.h"
#include "radvlm_hip.h"

namespace {

constexpr int CR_MAX_N = 262144;
constexpr int CR_SWEEP = 1024;               // columns per sweep step of the workgroup: four per thread

__global__ __launch_bounds__(256) void constrain_rows_kernel(float* __restrict__ x, long ld, int n, int* __restrict__ state, int state_rows,
                                                             const int* __restrict__ slot, const long long* __restrict__ tok,
                                                             const int* __restrict__ edge_off, const int* __restrict__ edge_tok,
                                                             const int* __restrict__ edge_next, int n_states, int n_edges) {
    __shared__ unsigned bits[CR_MAX_N / 32];
    __shared__ int sh;
    const int r = blockIdx.x, tid = threadIdx.x;
    const int si = slot ? slot[r] : r;
    const bool has_slot = si >= 0 && si < state_rows;
    int s = has_slot ? state[si] : -2;
    int lo = 0, hi = 0;                      // the edge run of a live s, clamped: 0 <= lo <= hi <= n_edges
    const bool live_in = s >= 0 && s < n_states;
    if (live_in) {
        lo = min(max(edge_off[s], 0), n_edges);
        hi = min(max(edge_off[s + 1], lo), n_edges);
    }
    if (tok && s >= 0) {                     // advance (uniform over the workgroup: every thread holds the same s, lo, hi)
        int next = -2;
        if (live_in) {
            const long long key = tok[r];
            while (hi - lo > 256) {          // 256-ary: the last probe <= key starts the piece that can hold the key
                const int step = (hi - lo + 255) / 256;
                if (tid == 0) sh = lo;
                __syncthreads();
                const long p = (long)lo + (long)tid * step;
                if (p < hi && (long long)edge_tok[p] <= key) atomicMax(&sh, (int)p);
                __syncthreads();
                lo = sh;
                hi = min(lo + step, hi);
                __syncthreads();
            }
            if (tid == 0) sh = -1;
            __syncthreads();
            if (lo + tid < hi && (long long)edge_tok[lo + tid] == key) sh = lo + tid;
            __syncthreads();
            if (sh >= 0) next = edge_next[sh];
            __syncthreads();
        }
        s = next;
        if (tid == 0 && has_slot) state[si] = s;
        lo = hi = 0;
        if (s >= 0 && s < n_states) {
            lo = min(max(edge_off[s], 0), n_edges);
            hi = min(max(edge_off[s + 1], lo), n_edges);
        }
    }
    if (s == -1) return;
    float* row = x + (long)r * ld;
    const bool dead = s < 0 || s >= n_states;    // no bit is read then: every column is banned
    if (!dead) {
        for (int w = tid; w < (n + 31) / 32; w += 256) bits[w] = 0u;
        __syncthreads();
        for (int e = lo + tid; e < hi; e += 256) {
            const int t = edge_tok[e];
            if (t >= n) break;
            if (t >= 0) atomicOr(&bits[t >> 5], 1u << (t & 31));
        }
        __syncthreads();
    }
    const bool vec = ((uintptr_t)row & 15) == 0;
    const f32x4 ninf = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int j = tid * 4; j < n; j += CR_SWEEP) {
        const unsigned keep = dead ? 0u : (bits[j >> 5] >> (j & 31)) & 15u;      // j % 4 == 0: the four bits lie in one word
        if (vec && keep == 0u && j + 3 < n) {
            *(f32x4*)(row + j) = ninf;
            continue;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (j + i < n && !((keep >> i) & 1u)) row[j + i] = -INFINITY;
    }
}

}  // namespace

extern "C" int rv_constrain_rows_f32(float* x, int64_t ld, int rows, int n, int32_t* state, int state_rows, const int32_t* slot,
                                     const int64_t* tok, const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next,
                                     int n_states, int n_edges, void* stream) {
    if (!x || !state || !edge_off || !edge_tok || !edge_next || rows < 1 || n < 1 || n > CR_MAX_N || ld < n) return RV_ERR_ARG;
    if (state_rows < 1 || (!slot && rows > state_rows) || n_states < 1 || n_edges < 1) return RV_ERR_ARG;
    hipLaunchKernelGGL(constrain_rows_kernel, dim3(rows), dim3(256), 0, ST, x, (long)ld, n, (int*)state, state_rows, (const int*)slot,
                       (const long long*)tok, (const int*)edge_off, (const int*)edge_tok, (const int*)edge_next, n_states, n_edges);
    return rv_check_launch();
}
