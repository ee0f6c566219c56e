// A4 (+A5/A6 fused), split operands, the 128-unit class (97-128 units): the default forward kernel of the benchmark model.
//
// Same mathematics as gru_split_kernel (gru_kernel.hip): U = U_hi + U_lo and h_{t-1} = h_hi + h_lo as fp16 pairs,
// U.h ~ U_hi.h_hi + U_hi.h_lo + U_lo.h_hi on the matrix cores with fp32 accumulation, the gate chain of gru_shared.h link
// for link.  What differs is the MFMA shape, where everything lives and when it is issued:
//   * v_mfma_f32_16x16x32_f16 (144 + 6 per wave and step).  The kernel runs at the chip's POWER wall, not at an issue or
//     pipe limit: the same instruction stream on all-zero operands takes 23 % less time, and at equal cycles per flop the
//     16x16x32 shape sustains 19 % more flop/s on random data than 32x32x16 (tools/ubench/mfma_shape_power.hip;
//     MI355X_MICROARCH.md, "DVFS give-back", item 7).  Tile: weights are the A operand (rows = units), the hidden tile the
//     B operand (columns = recurrent rows), D[unit][row]: a lane holds 4 consecutive units of ONE window's forward row and of
//     its reverse-complement row (sub-tiles: unit halves x row halves), so the gate math stays lane-local and a publish is
//     an 8-byte store per sub-tile.
//   * ONE wave per SIMD with the 512-register budget.  The 50 weight fragments of the wave's 32 units (U_hi, U_lo, Dense:
//     200 registers) are loaded ONCE, straight into the accumulation half of the register file (asm loads with AGPR
//     destinations), and every MFMA names them there: no copies, nothing streams, and the compiler's 256 architectural
//     VGPRs stay free for two tiles' accumulators and state.
//   * The input projection is not an MFMA: inputs are one-hot, so x.W + b is one of five rows.  The rows (exp2 domain,
//     both biases folded) sit in a 10 KB LDS table; a step's accumulators START as the table rows of the two bases of the
//     lane's window (forward and complemented reverse), read as the MFMA chain's C operand.
//   * TWO row tiles (2 x 16 windows) per workgroup, software-pipelined against each other: a "phase" is the 150 MFMAs of
//     one tile's step (X) with the whole epilogue of the other tile's step (Y) -- gate chains, fp16 hi/lo publish, the
//     workgroup barrier, table rows and first fragments of Y's next step -- and the softmax + max-merge of X's own logits of
//     two steps ago (stored while X was the epilogue tile, a barrier since: nothing in this phase feeds them), cut
//     into single operations and dropped into the gaps BETWEEN X's MFMAs (a wave issues in order; an MFMA holds the issue
//     port for 8 of its 16 cycles).  The barrier itself sits inside X's MFMA stream, four MFMAs from its end, and the last publish
//     stores two MFMAs in front of it: the barrier's s_waitcnt lgkmcnt(0) finds their LDS round trip already under way.
//   * The order of that interleave is generated (tools/gen_split2_schedule.py -> gru_split2_phase.inc) and pinned with
//     sched_barrier between gaps; the MFMAs are asm volatile, which the compiler keeps in program order.
//
// Inline-asm obligations (cdna_hip_programming.md 5.7) and how they are met -- by construction, and CHECKED on the compiler's
// output at every build (tools/lint_split2_isa.py, run by the Makefile): the register allocator is free to put a v_mov copy of an
// accumulator directly in front of the MFMA that takes it as C, and did so for one schedule variant (wrong results, no fault):
//   - an MFMA's result is read by compiler-scheduled code only many MFMAs later (the generator keeps the first gaps of a
//     phase free of anything that touches the previous phase's accumulators or Dense result);
//   - no MFMA operand is written by VALU code: fragments, table rows and Dense operands come straight from LDS reads, which
//     are the compiler's own loads (it waits for them in front of the asm statement);
//   - the weight loads are asm statements and so is the ONE s_waitcnt behind all 50 of them (volatile asm keeps its program order:
//     every MFMA stays behind it); the compiler's own counter waits only ever see more loads in flight than it knows of, never fewer.
//
// Launch shape: min(tile pairs, CUs) workgroups (a CU holds one: 146 KB of LDS, 512-register waves); weights and table are loaded once
// per workgroup, not once per pair.  Workgroup b starts with pair b; every later pair comes from the launch's queue (gru_params::queue:
// one word of the call's workspace, zero at the launch: pair = gridDim.x + its old value).  One lane asks for it in front of the drain,
// the answer goes through an LDS word behind the barrier that closes the pair: the round trip lies under the drain, and nothing of it
// lives across the time loop.  A pair costs every workgroup the same instructions but not the same time (a workgroup's XCD is fixed by
// its index and the XCDs need not hold one clock at the power cap), so a static share is balanced only on paper.  Without a queue
// (a caller that gave the entry point no workspace) workgroup b walks b, b + gridDim.x, ...; which workgroup runs a pair, and after
// which others, does not show in a bit of the result (max-merge, disjoint window rows).
#include "gru_shared.h"
#include <cstddef>
#include <mutex>
#include <type_traits>

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int NW = 4, UP = 128, KS = 4, HPAD = 16, HS = UP + HPAD;   // k-steps of 32; row pitch 144 halves: conflict-free ds_read_b128
constexpr int XT_PITCH = 4 * 128 * 4 + 32;                            // table row of one base: 4 kinds x 128 units fp32 + 32 B (bank spread)
constexpr int QUEUE_LDS = 16;                                         // behind the table: the word the next pair's index reaches the workgroup through

// Diagnostic build only (tools/build_split2_stamps.sh, -DDGRP_SPLIT2_STAMPS; never the product): per workgroup, words of 8 bytes in a
// buffer nothing else reads -- [0] s_memrealtime at entry, [1] at exit, [2] pairs run, then per pair s_memtime at set-up start,
// time-loop start, drain start and pair end.  One stamp per boundary, none inside the time loop; no output value depends on one.
#ifdef DGRP_SPLIT2_STAMPS
struct split2_stamp_buf { unsigned long long *at; int pairs_cap; int static_walk; };
split2_stamp_buf g_stamps = { nullptr, 0, 0 };
// (what a stamp needs is read where it is written -- buffer and capacity from the kernel-argument segment, the count of pairs run from
// an LDS word of the one lane that stamps -- so that the time loop carries nothing for it)
#define STAMP_DO(pair_k, slot, clock)                                                                                   \
    do {                                                                                                                \
        const unsigned long long t_ = (clock);                                                                          \
        const __attribute__((address_space(4))) unsigned *ks_ = (const __attribute__((address_space(4))) unsigned *)__builtin_amdgcn_kernarg_segment_ptr(); \
        asm volatile("" : "+s"(ks_));                                                                                   \
        unsigned long long *const sb_ = (unsigned long long *)(((uint64_t)ks_[offsetof(split2_args, stamps) / 4 + 1] << 32) | ks_[offsetof(split2_args, stamps) / 4]); \
        const unsigned cap_ = ks_[offsetof(split2_args, stamp_pairs) / 4];                                              \
        unsigned *const nrun_ = reinterpret_cast<unsigned *>(smem + ks_[offsetof(gru_params, xtab_off) / 4] + 5 * XT_PITCH + 4); \
        if (sb_ && wave == 0 && lane == 0) {                                                                            \
            unsigned long long *const row_ = sb_ + (size_t)blockIdx.x * (3 + 4 * (size_t)cap_);                         \
            if ((pair_k) < 0) {                                                                                         \
                if ((slot) == 0) *nrun_ = 0;                                                                            \
                row_[slot] = t_;                                                                                        \
                if ((slot) == 1) row_[2] = *nrun_;                                                                      \
            } else {                                                                                                    \
                const unsigned n_ = *nrun_;                                                                             \
                if (n_ < cap_) row_[3 + 4 * (size_t)n_ + (pair_k)] = t_;                                                \
                if ((pair_k) == 3) *nrun_ = n_ + 1;                                                                     \
            }                                                                                                           \
        }                                                                                                               \
    } while (0)
#define STAMP(slot, clock) STAMP_DO(-1, slot, clock)
#define STAMP_PAIR(k) STAMP_DO(k, 0, __builtin_amdgcn_s_memtime())
#else
#define STAMP(slot, clock) do { } while (0)
#define STAMP_PAIR(k) do { } while (0)
#endif

struct split2_weights {                   // 50 fragments = 200 AGPRs per lane, resident for the whole kernel
    u32x4 hi[3][KS][2], lo[3][KS][2];     // [gate r, g, z][k-step][unit half]: U_hi, U_lo
    u32x4 Bd_hi, Bd_lo;                   // Dense
};

// two fragments requested, not waited for: LOAD_WAIT behind the last LOAD2 (50 loads in flight: the counter holds 63)
#define LOAD2(a, pa, b, pb)                                                                                             \
    asm volatile("global_load_dwordx4 %0, %2, off\n\tglobal_load_dwordx4 %1, %3, off"                                   \
                 : "=&a"(a), "=&a"(b) : "v"(pa), "v"(pb) : "memory")
#define LOAD_WAIT asm volatile("s_waitcnt vmcnt(0)" ::: "memory")

// recurrent MFMA: A = weights (AGPR), B = hidden fragment; Dense MFMA: A = hidden rows, B = weights (AGPR)
#define MFMA_R(acc, Wf, b) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc) : "a"(Wf), "v"(b))
#define MFMA_D(acc, a, Wf) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "a"(Wf))
#define MFMA_DZ(acc, a, Wf) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=&v"(acc) : "v"(a), "a"(Wf))

struct tile_state {
    gru_params p;                         // batched records: the two tiles may belong to different records
    wg_ctx ctx;
    unsigned hcur, hnxt, lcur, lnxt;      // byte offsets of the hidden tiles (hi, lo; ping-pong) in the dynamic LDS
    unsigned myseq;                       // LDS byte offset of the class indices of window (lane & 15)
    float h[16];                          // gate state of the lane's 16 (row, unit) pairs: h, or h - 1 (ONERCP); element 4*sub + i
    f32x4 ar[4], ag[4], az[4], ax[4];     // pre-activations, sub-tile = 2 * unit half + row half (ax: the candidate's input projection)
    f32x4 dpl;                            // Dense partial logits of the previous step
    unsigned tabf, tabr;                  // LDS byte offsets of the table rows of the step in flight: forward base, complemented reverse base
    half8 f0h[2], f0l[2];                 // first fragments (k-step 0, row halves) of the NEXT contraction
    int p_off;                            // placement of the wave's logit register (reg = wave): row in the LDS image or -1
    int64_t p_row0;
    bool pr_on;
};

// a workgroup-uniform 64-bit value the compiler worked out on the vector unit, moved to scalar registers: what a tile keeps across the
// time loop (first window, first image row) must not take vector registers there
__device__ __forceinline__ int64_t split2_uniform(int64_t v)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(uint64_t)v), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// Set-up of ONE tile of a pair: what wg_setup (gru_shared.h) does for the one-tile kernels, for this kernel's carve, with wide
// accesses and WITHOUT the closing barrier -- the kernel runs it for both tiles of a pair and meets once.  Stages the class indices,
// zeroes h_{-1} (hi and lo tile) and the output image, writes the windows' placement.
// Sequences: the 16 windows of a tile cover ONE contiguous span of 15 s + T class indices.  Where that span (and up to 15 bytes of
// alignment shift) fits the [16][Tp] bytes of the carve, it is staged as it lies in HBM -- 16-byte loads between its unaligned ends,
// nothing outside [first byte of the first valid window, last byte of the last valid window] is read -- and window wi starts at byte
// seq_row0 + wi * s; otherwise (steps longer than a window) window by window at pitch Tp as in wg_setup.  Windows behind the last valid one
// then see whatever the bytes hold: every read is clamped to a table row and every output of theirs is masked.
// (LDS banks: the time loop's two byte reads per step go to wi * s + t.  At pitch Tp = 208 the 16 windows fall into 16 banks; in a span
// they do unless s is a multiple of 32 bytes -- s = 64 puts them into 4 banks, a 4-way conflict on 2 of a tile-step's ~50 LDS operations.
// Reasoned, not measured; the usual steps (50, 25, T / 4 of windows that are no multiple of 128) are conflict-free.)
template <int MODE>
__device__ __forceinline__ wg_ctx split2_tile_setup(const gru_params &p, unsigned char *base, int64_t bid, int tid, unsigned &seq_row0, unsigned &seq_pitch)
{
    wg_ctx c;
    c.hbuf = reinterpret_cast<_Float16 *>(base);
    c.dpart = reinterpret_cast<float *>(base + gru_lds_hbuf(UP, HPAD));
    c.seqs = base + gru_lds_hbuf(UP, HPAD) + gru_lds_dpart(NW);
    c.row0s = reinterpret_cast<int64_t *>(c.seqs + gru_lds_seq(p.Tp));
    c.rowoff = reinterpret_cast<int *>(c.row0s + DGRP_WG_WINDOWS);
    c.obuf = reinterpret_cast<unsigned *>(c.rowoff + DGRP_WG_WINDOWS);
    const int T = p.T, C = p.C;
    c.wg_w = split2_uniform(p.w0 + bid * DGRP_WG_WINDOWS);
    c.nvalid = __builtin_amdgcn_readfirstlane((int)min((int64_t)DGRP_WG_WINDOWS, p.w0 + p.nw - c.wg_w));
    if ((DGRP_WG_WINDOWS - 1) * p.s + T + 15 <= (int64_t)DGRP_WG_WINDOWS * p.Tp) {
        const uint8_t *src = p.idx + c.wg_w * p.s;                                   // (not dereferenced without a valid window)
        const int have = c.nvalid > 0 ? (c.nvalid - 1) * (int)p.s + T : 0;           // bytes of the valid windows
        const int sh = (int)(reinterpret_cast<uintptr_t>(src) & 15);
        const int head = min(have, (16 - sh) & 15);                                  // bytes in front of the first aligned 16
        const int nbody = (have - head) >> 4, tail0 = head + 16 * nbody;
#pragma nounroll
        for (int i = tid; i < nbody; i += 64 * NW)
            *reinterpret_cast<uint4 *>(c.seqs + sh + head + 16 * i) = *reinterpret_cast<const uint4 *>(src + head + 16 * i);
#pragma nounroll
        for (int i = tid; i < head + have - tail0; i += 64 * NW) {
            const int j = i < head ? i : tail0 + (i - head);
            c.seqs[sh + j] = src[j];
        }
        seq_row0 = (unsigned)sh;
        seq_pitch = (unsigned)p.s;
    } else {
#pragma nounroll
        for (int i = tid; i < DGRP_WG_WINDOWS * T; i += 64 * NW) {
            const int wi = i / T, t = i - wi * T;
            c.seqs[wi * p.Tp + t] = wi < c.nvalid ? p.idx[(c.wg_w + wi) * p.s + t] : (uint8_t)4;
        }
        seq_row0 = 0;
        seq_pitch = (unsigned)p.Tp;
    }
    unsigned z0 = 0u;
    asm volatile("" : "+v"(z0));                                                     // (a constant would be kept in four registers across the time loop)
    const uint4 zero = { z0, z0, z0, z0 };
#pragma nounroll
    for (int i = tid; i < 32 * HS * 2 / 16; i += 64 * NW) {                           // h_{-1} = 0: first tile of each ping-pong
        reinterpret_cast<uint4 *>(base)[i] = zero;
        reinterpret_cast<uint4 *>(base + p.lo_tile_off)[i] = zero;
    }
    c.lo = 0;
    if (MODE == 0) {
        // smallest placement row of the two ends; windows that fall outside [lo, lo + ospan) go to HBM directly (wg_setup)
        const int64_t a = dgrp_place_row(p.place, c.wg_w, p.s), b = dgrp_place_row(p.place, c.wg_w + c.nvalid - 1, p.s);
        c.lo = split2_uniform(a < b ? a : b);
        const int words = p.ospan * C;                                               // (the image starts on a 16-byte boundary of the carve)
#pragma nounroll
        for (int i = tid; i < words / 4; i += 64 * NW) reinterpret_cast<uint4 *>(c.obuf)[i] = zero;
        if (tid < (words & 3)) c.obuf[(words & ~3) + tid] = 0u;
    }
    if (tid < DGRP_WG_WINDOWS) {
        int64_t r0 = -1;
        int off = -1;
        if (tid < c.nvalid) {
            r0 = MODE == 0 ? dgrp_place_row(p.place, c.wg_w + tid, p.s) : (c.wg_w + tid - p.w0 + p.avgw) * (int64_t)T;
            if (MODE == 0 && r0 >= c.lo && r0 - c.lo + T <= p.ospan) off = (int)(r0 - c.lo);
        }
        c.row0s[tid] = r0;
        c.rowoff[tid] = off;
    }
    return c;
}

// The kernel's ONE argument: it is the kernel-argument segment from byte 0 on, and the pair loop re-reads its members from there
// (offsetof below) instead of keeping them in registers across the time loop.
struct split2_args {
    gru_params p;
    int half_bytes;                       // bytes of one tile's LDS carve
    int npairs;                           // tile pairs of the launch
#ifdef DGRP_SPLIT2_STAMPS
    unsigned long long *stamps;
    int stamp_pairs;
#endif
};

template <int MODE, bool ONERCP>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) gru_split2_kernel(const split2_args args)
{
    static_assert(offsetof(split2_args, p) == 0 && sizeof(gru_params) % 4 == 0 && offsetof(split2_args, half_bytes) % 4 == 0 &&
                  offsetof(split2_args, npairs) % 4 == 0 && offsetof(gru_params, queue) % 8 == 0, "the pair loop reads the argument as 32-bit words");
    const gru_params &pin = args.p;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int T = pin.T, C = pin.C;
    STAMP(0, __builtin_amdgcn_s_memrealtime());

    split2_weights W;
    {
        const uint4 *p16 = pin.pack16 + (size_t)wave * 48 * 64 + lane;        // [(pass*3 + gate)*8 + kstep*2 + unit half][64]
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                LOAD2(W.hi[g][ks][0], p16 + (size_t)(g * 8 + ks * 2) * 64, W.hi[g][ks][1], p16 + (size_t)(g * 8 + ks * 2 + 1) * 64);
                LOAD2(W.lo[g][ks][0], p16 + (size_t)(24 + g * 8 + ks * 2) * 64, W.lo[g][ks][1], p16 + (size_t)(24 + g * 8 + ks * 2 + 1) * 64);
            }
        const uint4 *mypack = pin.pack + (size_t)wave * pin.nfrag * 64 + lane;    // Dense fragments of the 32x32 pack (api.hip): same shape
        LOAD2(W.Bd_hi, mypack + (size_t)(3 * (2 * KS + 1) + 1) * 64, W.Bd_lo, mypack + (size_t)(3 * (2 * KS + 1) + 2) * 64);
        LOAD_WAIT;
    }
    // the input-projection table: [5 bases][4 kinds][128 units] fp32 -> LDS rows of XT_PITCH bytes
    for (int i = tid; i < 5 * 512; i += 256)
        *reinterpret_cast<float *>(smem + pin.xtab_off + (i / 512) * XT_PITCH + (i % 512) * 4) = pin.xtab[i];

    const int wi = lane & 15, q4 = lane >> 4;                     // window of this lane; its k-group / unit group
    const int cls = lane & 15;
    const float fbias = cls < C ? pin.ffb[cls] : 0.0f;
    const unsigned frag_lane = (unsigned)(wi * HS + 8 * q4) * 2;                            // fragment: row wi (+16: its reverse complement), k 8 q4 ..
    const unsigned dense_lane = (unsigned)(wi * HS + 32 * wave + 8 * q4) * 2;
    const unsigned pub_lane = (unsigned)(wi * HS + 32 * wave + 4 * q4) * 2;                 // publish: 4 units 32 w + 16 uh + 4 q4 ..
    const unsigned tab_lane = (unsigned)pin.xtab_off + (unsigned)(32 * wave + 4 * q4) * 4;  // table: the same 4 units, + 64 B per unit half

    tile_state S0, S1;                      // two named objects, never indexed: they must stay in registers
    auto setup = [&](tile_state &Z, const gru_params &pk, int tid_k, int half_k, int pair, int x) {
        unsigned char *base = smem + (size_t)x * half_k;
        Z.p = pk;
        const int64_t bid = wg_record_at<MODE>(pk, Z.p, 2 * (int64_t)pair + x);
        unsigned seq_row0, seq_pitch;
        Z.ctx = split2_tile_setup<MODE>(Z.p, base, bid, tid_k, seq_row0, seq_pitch);  // no barrier: the caller meets once for both tiles
        Z.hcur = (unsigned)x * half_k;                            // hbuf is the first item of the carve
        Z.hnxt = Z.hcur + 32 * HS * 2;
        Z.lcur = (unsigned)x * half_k + pk.lo_tile_off;
        Z.lnxt = Z.lcur + 32 * HS * 2;
        Z.myseq = (unsigned)(Z.ctx.seqs - smem) + seq_row0 + (tid_k & 15) * seq_pitch;
#pragma unroll
        for (int i = 0; i < 16; ++i) Z.h[i] = ONERCP ? -1.0f : 0.0f;
    };
    // what setup leaves in LDS for the lane (read behind the barrier)
    auto placement = [&](tile_state &Z, int tid_k) {
        const int pwi_k = 4 * ((tid_k & 63) >> 4) + wave;
        Z.p_off = Z.ctx.rowoff[pwi_k];
        Z.p_row0 = Z.ctx.row0s[pwi_k];
        Z.pr_on = cls < C && pwi_k < Z.ctx.nvalid;
    };

    auto lds16 = [&](unsigned off) -> half8 { return *reinterpret_cast<const half8 *>(smem + off); };
    auto ldsf4 = [&](unsigned off) -> f32x4 { return *reinterpret_cast<const f32x4 *>(smem + off); };
    // table rows of step tn for this lane's window: forward base seq[tn]; reverse strand base comp(seq[T-1-tn]), complement
    // table [3,2,1,0,4] (model.py:233-237)
    auto tab_rows = [&](tile_state &Z, uint32_t bf, uint32_t br) {
        bf = bf < 4 ? bf : 4;                                     // (the step behind the last one reads a byte outside the window)
        br = br < 4 ? 3 - br : 4;
        Z.tabf = tab_lane + bf * XT_PITCH;
        Z.tabr = tab_lane + br * XT_PITCH;
    };
    // accumulators of the next step start as the table rows (kinds 0 r, 1 g, 2 z); sub-tile = 2 * unit half + row half
    auto acc_init = [&](tile_state &Z, int g, int sub) {
        const f32x4 v = ldsf4(((sub & 1) ? Z.tabr : Z.tabf) + g * 512 + (sub >> 1) * 64);
        if (g == 0) Z.ar[sub] = v; else if (g == 1) Z.ag[sub] = v; else Z.az[sub] = v;
    };

    // ---- one phase: tile X's step tx on the matrix pipe, tile Y's epilogue of step ty in the gaps --------------------
    struct frag_ring { half8 h[2][2], l[2][2]; };                 // [k-step parity][row half]
    struct dense_ops { half8 a0, a1, l0, l1; };
    struct fin_state { float d[NW], lg, m, e, s; };
    auto phase = [&](auto do_x, auto do_y, auto do_f, tile_state &X, tile_state &Y, int tx, int ty) __attribute__((always_inline)) {
        constexpr bool DO_X = decltype(do_x)::value, DO_Y = decltype(do_y)::value, DO_F = decltype(do_f)::value;
        frag_ring F;
        dense_ops D;
        fin_state fs;
        split_gate_tmp gt[16];
        float pbh[4][4];
        uint2 pbhv[4], pblv[4];
        uint32_t xp_bf = 4, xp_br = 4;
        const int td = ty - 1;                                    // step whose Dense partials Y stores in this phase
        const int tf = tx - 2;                                    // step whose logits X finishes in this phase (stored one phase ago, a barrier since)
        if constexpr (DO_X) { F.h[0][0] = X.f0h[0]; F.h[0][1] = X.f0h[1]; F.l[0][0] = X.f0l[0]; F.l[0][1] = X.f0l[1]; }
#define GAP __builtin_amdgcn_sched_barrier(0);
        // MFMA n (0..35) of k-step ks: pass n / 12 (hi.h_hi, hi.h_lo, lo.h_hi), then gate, unit half, row half (two in a row share
        // the A fragment)
#define M_K(ks, n)                                                                                               \
    if constexpr (DO_X) {                                                                                        \
        constexpr int ps_ = (n) / 12, g_ = ((n) % 12) / 4, uh_ = ((n) % 4) / 2, rh_ = (n) % 2, sub_ = 2 * uh_ + rh_; \
        const half8 &b_ = ps_ == 1 ? F.l[(ks) & 1][rh_] : F.h[(ks) & 1][rh_];                                    \
        const u32x4 &w_ = ps_ == 2 ? W.lo[g_][ks][uh_] : W.hi[g_][ks][uh_];                                      \
        if constexpr (g_ == 0) MFMA_R(X.ar[sub_], w_, b_);                                                       \
        else if constexpr (g_ == 1) MFMA_R(X.ag[sub_], w_, b_);                                                  \
        else MFMA_R(X.az[sub_], w_, b_);                                                                         \
    }
#define M_D(i)                                                                                                   \
    if constexpr (DO_X) {                                                                                        \
        if constexpr ((i) == 0) MFMA_DZ(X.dpl, D.a0, W.Bd_hi);                                                   \
        else if constexpr ((i) == 1) MFMA_D(X.dpl, D.a1, W.Bd_hi);                                               \
        else if constexpr ((i) == 2) MFMA_D(X.dpl, D.a0, W.Bd_lo);                                               \
        else if constexpr ((i) == 3) MFMA_D(X.dpl, D.a1, W.Bd_lo);                                               \
        else if constexpr ((i) == 4) MFMA_D(X.dpl, D.l0, W.Bd_hi);                                               \
        else MFMA_D(X.dpl, D.l1, W.Bd_hi);                                                                       \
    }
        // fragments of k-step ks of X's hidden tile (requested one k-step ahead): both row halves, hi and lo
#define PF(ks)                                                                                                   \
    if constexpr (DO_X) {                                                                                        \
        F.h[(ks) & 1][0] = lds16(X.hcur + frag_lane + 64 * (ks)); F.h[(ks) & 1][1] = lds16(X.hcur + frag_lane + 16 * HS * 2 + 64 * (ks)); \
        F.l[(ks) & 1][0] = lds16(X.lcur + frag_lane + 64 * (ks)); F.l[(ks) & 1][1] = lds16(X.lcur + frag_lane + 16 * HS * 2 + 64 * (ks)); \
    }
        // Dense operands of X: h_{tx-1} of the wave's 32 units, window rows and their reverse complements (= the Average)
#define RDD                                                                                                      \
    if constexpr (DO_X) {                                                                                        \
        D.a0 = lds16(X.hcur + dense_lane); D.a1 = lds16(X.hcur + dense_lane + 16 * HS * 2);                      \
        D.l0 = lds16(X.lcur + dense_lane); D.l1 = lds16(X.lcur + dense_lane + 16 * HS * 2);                      \
        if (MODE == 2 && tx > 0 && (lane & 15) < X.ctx.nvalid)                                                   \
            split_avg_store(X.p, X.ctx.wg_w, tx - 1, UP, wave, D.a0, D.a1, D.l0, D.l1);                          \
    }
        // ---- Y's epilogue ------------------------------------------------------------------------------------
        // the candidate's input projection of the step being finished (table kind 3), sub-tile by sub-tile
#define AXL(sub) \
    if constexpr (DO_Y) Y.ax[sub] = ldsf4((((sub) & 1) ? Y.tabr : Y.tabf) + 3 * 512 + ((sub) >> 1) * 64);
#define DS(i)                                                                                                    \
    if constexpr (DO_Y) Y.ctx.dpart[((size_t)(td & 1) * 4 * NW + wave) * 64 + lane + (i) * NW * 64] = Y.dpl[i];
#define G(e, op) \
    if constexpr (DO_Y) split_gate_op<ONERCP, op>(gt[e], Y.ar[(e) / 4][(e) % 4], Y.ag[(e) / 4][(e) % 4], Y.az[(e) / 4][(e) % 4], Y.ax[(e) / 4][(e) % 4], Y.h[e]);
        // publish sub-tile g = 2 * unit half + row half: 4 consecutive units of row 16 rh + (lane & 15)
#define PB(g, op)                                                                                                \
    if constexpr (DO_Y) {                                                                                        \
        if constexpr ((op) == 0) {                                                                               \
            pbh[g][0] = split_state_h<ONERCP>(Y.h[4 * (g)]); pbh[g][1] = split_state_h<ONERCP>(Y.h[4 * (g) + 1]); \
            pbh[g][2] = split_state_h<ONERCP>(Y.h[4 * (g) + 2]); pbh[g][3] = split_state_h<ONERCP>(Y.h[4 * (g) + 3]); \
        } else if constexpr ((op) == 1) {                                                                        \
            pbhv[g] = split_pack4(pbh[g]);                                                                       \
        } else if constexpr ((op) == 2) {                                                                        \
            split_residual4(pbh[g], pbhv[g]);                                                                    \
        } else if constexpr ((op) == 3) {                                                                        \
            pblv[g] = split_pack4(pbh[g]);                                                                       \
        } else {                                                                                                 \
            *reinterpret_cast<uint2 *>(smem + Y.hnxt + pub_lane + ((g) & 1) * 16 * HS * 2 + ((g) >> 1) * 32) = pbhv[g]; \
            *reinterpret_cast<uint2 *>(smem + Y.lnxt + pub_lane + ((g) & 1) * 16 * HS * 2 + ((g) >> 1) * 32) = pblv[g]; \
        }                                                                                                        \
    }
        // h_t of Y is complete in LDS: meet the other waves, then flip Y's ping-pong
#define BAR                                                                                                      \
    if constexpr (DO_Y) {                                                                                        \
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");                                          \
        unsigned sw_ = Y.hcur; Y.hcur = Y.hnxt; Y.hnxt = sw_;                                                    \
        sw_ = Y.lcur; Y.lcur = Y.lnxt; Y.lnxt = sw_;                                                             \
    }
        // Y's next step: first fragments, the two bases of the lane's window and their table rows, the accumulators' start
#define RD0                                                                                                      \
    if constexpr (DO_Y) {                                                                                        \
        Y.f0h[0] = lds16(Y.hcur + frag_lane); Y.f0h[1] = lds16(Y.hcur + frag_lane + 16 * HS * 2);                \
        Y.f0l[0] = lds16(Y.lcur + frag_lane); Y.f0l[1] = lds16(Y.lcur + frag_lane + 16 * HS * 2);                \
    }
#define XP(op)                                                                                                   \
    if constexpr (DO_Y) {                                                                                        \
        if constexpr ((op) == 0) { xp_bf = smem[Y.myseq + ty + 1]; xp_br = smem[Y.myseq + T - 2 - ty]; }                       \
        else tab_rows(Y, xp_bf, xp_br);                                                                          \
    }
#define CI(g, sub) \
    if constexpr (DO_Y) acc_init(Y, g, sub);
        // softmax + merge of step tf's logits of tile X (its partials were stored while X was the epilogue tile, one phase and one
        // barrier ago) for the wave's register (window = 4*(lane>>4) + wave, class = lane & 15)
#define FN(op)                                                                                                   \
    if constexpr (DO_F) {                                                                                        \
        if constexpr ((op) == 0) {                                                                               \
            const float *dp_ = X.ctx.dpart + ((size_t)(tf & 1) * 4 + wave) * NW * 64 + lane;                     \
            fs.d[0] = dp_[0]; fs.d[1] = dp_[64]; fs.d[2] = dp_[128]; fs.d[3] = dp_[192];                         \
        } else if constexpr ((op) == 1) {                                                                        \
            const float sum_ = ((fs.d[0] + fs.d[1]) + fs.d[2]) + fs.d[3];                                        \
            fs.lg = cls < C ? sum_ + fbias : -INFINITY;                                                          \
        } else if constexpr ((op) == 2) { if (MODE != 2) fs.m = row_max_ror<8>(fs.lg); }                         \
        else if constexpr ((op) == 3) { if (MODE != 2) fs.m = row_max_ror<4>(fs.m); }                            \
        else if constexpr ((op) == 4) { if (MODE != 2) fs.m = row_max_ror<2>(fs.m); }                            \
        else if constexpr ((op) == 5) { if (MODE != 2) fs.m = row_max_ror<1>(fs.m); }                            \
        else if constexpr ((op) == 6) { if (MODE != 2) fs.e = __builtin_amdgcn_exp2f(1.4426950408889634f * (fs.lg - fs.m)); } \
        else if constexpr ((op) == 7) { if (MODE != 2) fs.s = fs.e + row_ror<8>(fs.e); }                         \
        else if constexpr ((op) == 8) { if (MODE != 2) fs.s += row_ror<4>(fs.s); }                               \
        else if constexpr ((op) == 9) { if (MODE != 2) fs.s += row_ror<2>(fs.s); }                               \
        else if constexpr ((op) == 10) { if (MODE != 2) fs.s += row_ror<1>(fs.s); }                              \
        else if constexpr ((op) == 11) { if (MODE != 2) fs.e *= __builtin_amdgcn_rcpf(fs.s); }                   \
        else { if (X.pr_on && tf >= 0) emit_value<MODE>(X.p, X.ctx, X.p_off, X.p_row0, tf, cls, MODE == 2 ? fs.lg : fs.e); } \
    }
#include "gru_split2_phase.inc"
#undef GAP
#undef M_K
#undef M_D
#undef PF
#undef RDD
#undef AXL
#undef DS
#undef G
#undef PB
#undef BAR
#undef RD0
#undef XP
#undef CI
#undef FN
    };
    const std::true_type yes;
    const std::false_type no;

    // prologue: the operands of both tiles' step 0 (h_{-1} = 0 is in LDS), then tile 0's step 0 with nothing beside it
    auto first_step = [&](tile_state &Z) {
        tab_rows(Z, smem[Z.myseq], smem[Z.myseq + T - 1]);
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int sub = 0; sub < 4; ++sub) acc_init(Z, g, sub);
        Z.f0h[0] = lds16(Z.hcur + frag_lane); Z.f0h[1] = lds16(Z.hcur + frag_lane + 16 * HS * 2);
        Z.f0l[0] = lds16(Z.lcur + frag_lane); Z.f0l[1] = lds16(Z.lcur + frag_lane + 16 * HS * 2);
    };
    for (int pair = blockIdx.x;;) {
    // A pair's set-up is a few hundred instructions in front of 2 T phases that leave no register free.  What it needs is taken afresh for
    // every pair -- the launch parameters from the kernel-argument segment (= `args`, the kernel's only argument), the thread index
    // through an opaque copy -- so that nothing of it is hoisted out of this loop and carried, spilled, across the time loop.
    const __attribute__((address_space(4))) unsigned *kargs = (const __attribute__((address_space(4))) unsigned *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kargs));
    struct { unsigned w[sizeof(gru_params) / 4]; } kraw;
#pragma unroll
    for (unsigned i = 0; i < sizeof(gru_params) / 4; ++i) kraw.w[i] = kargs[offsetof(split2_args, p) / 4 + i];   // (scalar loads; members nothing reads are not loaded)
    const gru_params pk = __builtin_bit_cast(gru_params, kraw);
    const int half_k = (int)kargs[offsetof(split2_args, half_bytes) / 4];
    int tid_k = 64 * wave + lane;                // (= tid, from what the time loop keeps anyway)
    asm volatile("" : "+v"(tid_k));
    STAMP_PAIR(0);
    setup(S0, pk, tid_k, half_k, pair, 0);
    setup(S1, pk, tid_k, half_k, pair, 1);
    __syncthreads();
    placement(S0, tid_k);
    placement(S1, tid_k);
    first_step(S0);
    first_step(S1);
    STAMP_PAIR(1);
    phase(yes, no, no, S0, S1, 0, 0);
    // Register copies the allocator places on a control-flow edge (loop entry, back edge, exit) are VALU reads it does not know to
    // keep away from the asm MFMAs in front of them: the last MFMAs of a phase have to be complete before the edge.
#define EDGE_PAD do { asm volatile("s_nop 15\n\ts_nop 7"); __builtin_amdgcn_sched_barrier(0); } while (0)
    EDGE_PAD;
    for (int t = 0; t + 1 < T; ++t) {
        phase(yes, yes, yes, S1, S0, t, t);          // tile 1's step t      ||  tile 0 finishes step t
        phase(yes, yes, yes, S0, S1, t + 1, t);      // tile 0's step t + 1  ||  tile 1 finishes step t
        EDGE_PAD;
    }
    phase(yes, yes, yes, S1, S0, T - 1, T - 1);
    phase(no, yes, yes, S0, S1, T, T - 1);      // (tile 0's logits of step T - 2 are finished here; tile 1's in its drain)

    // drain: Dense and softmax/merge of the last step, image flush
    auto drain = [&](tile_state &Z, bool prev_open, int tid_d) {
        const int lane_d = tid_d & 63;
        const half8 a0 = lds16(Z.hcur + dense_lane), a1 = lds16(Z.hcur + dense_lane + 16 * HS * 2);
        const half8 l0 = lds16(Z.lcur + dense_lane), l1 = lds16(Z.lcur + dense_lane + 16 * HS * 2);
        if (MODE == 2 && (lane_d & 15) < Z.ctx.nvalid) split_avg_store_lane(Z.p, Z.ctx.wg_w, T - 1, UP, wave, lane_d, a0, a1, l0, l1);
        f32x4 d;
        MFMA_DZ(d, a0, W.Bd_hi); MFMA_D(d, a1, W.Bd_hi); MFMA_D(d, a0, W.Bd_lo); MFMA_D(d, a1, W.Bd_lo); MFMA_D(d, l0, W.Bd_hi); MFMA_D(d, l1, W.Bd_hi);
        asm volatile("s_nop 15\n\ts_nop 7" : "+v"(d));           // MFMA result -> VALU/LDS read, no compiler padding behind asm
        float *dw = Z.ctx.dpart + ((size_t)((T - 1) & 1) * 4 * NW + wave) * 64 + lane_d;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) dw[reg * NW * 64] = d[reg];
        __syncthreads();
        if (prev_open && T > 1) finish_register<NW, MODE>(Z.p, Z.ctx, T - 2, wave, fbias, Z.p_off, Z.p_row0, lane_d);
        finish_register<NW, MODE>(Z.p, Z.ctx, T - 1, wave, fbias, Z.p_off, Z.p_row0, lane_d);
        if (MODE == 0 && Z.p.ospan > 0) flush_image<NW>(Z.p, Z.ctx, tid_d);
    };
    int tid_d = 64 * wave + lane;
    asm volatile("" : "+v"(tid_d));             // (nothing of the drain is worked out ahead of the time loop and kept across it)
    STAMP_PAIR(2);
    // the next pair: ONE lane asks the queue in front of the drain (the counter's round trip lies under it: the drain has registers to
    // spare, the time loop has none) and hands the answer to the workgroup through an LDS word in front of the closing barrier
    const __attribute__((address_space(4))) unsigned *kargs_d = kargs;
    asm volatile("" : "+s"(kargs_d));           // (read here, not ahead of the time loop)
    typedef __attribute__((address_space(1))) unsigned global_u32;
    global_u32 *const queue = (global_u32 *)(((uint64_t)kargs_d[offsetof(gru_params, queue) / 4 + 1] << 32) | kargs_d[offsetof(gru_params, queue) / 4]);
    unsigned *const qword = reinterpret_cast<unsigned *>(smem + kargs_d[offsetof(gru_params, xtab_off) / 4] + 5 * XT_PITCH);
    const bool ask = queue && tid_d == 0;
    unsigned nxt;
    asm volatile("" : "=v"(nxt));               // (no value: only the asking lane's is read, and nothing waits for the answer here)
    // (an increment that never wraps, not an add: the compiler would fold an add over the wave's lanes and wait for the answer at once)
    if (ask) nxt = __builtin_amdgcn_atomic_inc32(queue, 0xffffffffu, __ATOMIC_RELAXED, "agent");
    drain(S0, false, tid_d);
    drain(S1, true, tid_d);                            // tile 1 stored its partials of step T - 2 in the last phase: no phase of its own follows
    if (ask) *qword = nxt + gridDim.x;
    __syncthreads();                            // the next pair's set-up rewrites what this pair's drain and flush still read
    EDGE_PAD;                                   // (the pair loop's back edge and exit: the drain's Dense chain has its own pad; kept as the rule)
    STAMP_PAIR(3);
    if (queue) pair = __builtin_amdgcn_readfirstlane((int)*qword);          // (written once per pair, read behind the barrier: no set-up touches it)
    else pair += (int)gridDim.x;
    if (pair >= (int)kargs_d[offsetof(split2_args, npairs) / 4]) break;
    }
    STAMP(1, __builtin_amdgcn_s_memrealtime());
}

// compute units of the current device, looked up once per DEVICE (records run on a pool of host threads, ranks on devices of their own)
static int split2_cu_count(int *cus)
{
    static std::mutex mu;
    static int known[64];                    // 0 = not asked yet
    int dev = 0;
    DGRP_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    if (dev < 0 || dev >= 64 || known[dev] == 0) {
        int n = 0;
        DGRP_HIP(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
        if (n < 1) n = 1;
        if (dev < 0 || dev >= 64) { *cus = n; return DGRP_OK; }
        known[dev] = n;
    }
    *cus = known[dev];
    return DGRP_OK;
}

template <int MODE, bool ONERCP>
int launch_split2(const gru_params &p, int64_t groups, int half_bytes, hipStream_t stream)
{
    static std::once_flag configured;        // (records run on a pool of host threads: an unsynchronised flag was a data race)
    static hipError_t cfg_err = hipSuccess;
    std::call_once(configured, [] { cfg_err = hipFuncSetAttribute((const void *)gru_split2_kernel<MODE, ONERCP>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); });
    DGRP_HIP(cfg_err);
    // a CU holds ONE workgroup (LDS, registers): as many workgroups as CUs, each walking its share of the tile pairs (any grid gives the
    // same bits; one larger than the CUs at hand is merely less balanced)
    const int64_t npairs = (groups + 1) / 2;
    int cus = 0;
    if (const int rc = split2_cu_count(&cus)) return rc;
    const int64_t grid = npairs < cus ? npairs : cus;
    DGRP_REQUIRE(npairs >= 1 && npairs <= 0x7fff0000, "gru_split2_kernel: tile pairs out of range");      // (the walk counts pairs in an int)
    // the queue: only a launch with more pairs than workgroups hands any out (short records pay no second launch); zeroed on THIS stream
    split2_args a{ p, half_bytes, (int)npairs };
    if (npairs <= grid) a.p.queue = nullptr;
#ifdef DGRP_SPLIT2_STAMPS
    if (g_stamps.static_walk) a.p.queue = nullptr;
    a.stamps = g_stamps.at;
    a.stamp_pairs = g_stamps.pairs_cap;
#endif
    if (a.p.queue) DGRP_HIP(hipMemsetAsync(a.p.queue, 0, sizeof(unsigned), stream));
    hipLaunchKernelGGL((gru_split2_kernel<MODE, ONERCP>), dim3((unsigned)grid), dim3(256), (size_t)2 * half_bytes + 5 * XT_PITCH + QUEUE_LDS, stream, a);
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}

}  // namespace

#ifdef DGRP_SPLIT2_STAMPS
// diagnostic build: where the next launches write their stamps (3 + 4 pairs_cap words of 8 bytes per workgroup, zeroed by the caller;
// NULL: nowhere), and whether they walk the static stride although the call has a queue
extern "C" __attribute__((visibility("default"))) int dgrp_split2_stamps(void *d_buf, int pairs_cap, int static_walk)
{
    g_stamps = { (unsigned long long *)d_buf, pairs_cap, static_walk };
    return DGRP_OK;
}
#endif

int dgrp_split2_launch(const gru_params &p, int64_t groups, int half_bytes, bool onercp, hipStream_t stream)
{
    if (onercp)
        return p.mode == 0 ? launch_split2<0, true>(p, groups, half_bytes, stream)
             : p.mode == 1 ? launch_split2<1, true>(p, groups, half_bytes, stream) : launch_split2<2, true>(p, groups, half_bytes, stream);
    return p.mode == 0 ? launch_split2<0, false>(p, groups, half_bytes, stream)
         : p.mode == 1 ? launch_split2<1, false>(p, groups, half_bytes, stream) : launch_split2<2, false>(p, groups, half_bytes, stream);
}
