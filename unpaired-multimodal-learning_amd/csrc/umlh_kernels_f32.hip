// fp32 (parity-mode) kernels of the UML head step for gfx950.
//
// All matrix work runs on the f32-input MFMA v_mfma_f32_32x32x2_f32, which is
// bit-for-bit a k-ordered fp32 fma chain (MI355X guide, "FP32-input MFMA"), so
// logits/loss/gradients agree with the reference's fp32 PyTorch path to fp32
// reduction-order noise (<1e-4 on logits, the north_star tolerance).
//
//   fwd_ce_f32     fused  features x W^T * scale -> softmax-CE -> dZ^T, per-row
//                  loss / top-1 / d(scale)   (head.py:77-84, finetune.py:186-188,197-198)
//   gemm_f32       generic tiled GEMM with row gathers and split-K slabs: img_proj
//                  forward, dW = dZ^T F, dH^T = W^T dZ^T, dW_proj = dH^T X
//   reduce_update  sum split-K slabs (+ optimizer step in the same pass)
//   finalize       per-step scalars + the two learnable logit scales
//   zero_shot      head.py:22-37
#include "umlh_common.h"
#include "umlh_launch.h"
#include "umlh_feistel.h"
#include <cstdlib>

// timing-only ablations exist for kernel analysis and are compiled in only with -DUMLH_ABLATIONS (see umlh_kernels_bf16.hip)
#ifdef UMLH_ABLATIONS
#define UMLH_ABL(cond) (cond)
#else
#define UMLH_ABL(cond) (false)
#endif

// --------------------------------------------------------------------------- //
// staging helpers: global -> registers -> LDS, k-major LDS tiles [KT][LD]
// --------------------------------------------------------------------------- //
// Load 4 consecutive floats p[0..3] with element guards lim (number of valid
// elements from p, may be <= 0); vector path when 16-B aligned and fully valid.
__device__ __forceinline__ f32x4v load4_guard(const float* p, int lim, bool vec_ok) {
    f32x4v v = {0.f, 0.f, 0.f, 0.f};
    if (lim >= 4 && vec_ok) {
        v = *reinterpret_cast<const f32x4v*>(p);
    } else {
        if (lim > 0) v[0] = p[0];
        if (lim > 1) v[1] = p[1];
        if (lim > 2) v[2] = p[2];
        if (lim > 3) v[3] = p[3];
    }
    return v;
}

// --------------------------------------------------------------------------- //
// x3 products (umlh_f32_x3, umlh_common.h): both fp32 operands split into three bf16 piece planes (0 = hi, 1 = mid, 2 = lo),
// six piece products per product on v_mfma_f32_32x32x16_bf16.  X3_ORDER is the order they are issued in, {plane of A, plane
// of B}: small terms first, the hi*hi product last.  gemm_f32, dw_f32x3 and the forward's MODE 3 all read it (and
// tests/_gemm_ref.py restates it as X3_PAIRS).
// --------------------------------------------------------------------------- //
constexpr int X3_ORDER[6][2] = {{2, 0}, {0, 2}, {1, 1}, {1, 0}, {0, 1}, {0, 0}};   // lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi
typedef unsigned int u32x4s __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// element i of the three planes p[0..2] <- the pieces of the pair (x, y)
__device__ __forceinline__ void split3_into(u32x4s (&p)[3], int i, float x, float y) {
    const Split3 s3 = split3_pair(x, y);
    p[0][i] = s3.hi; p[1][i] = s3.mid; p[2][i] = s3.lo;
}

// --------------------------------------------------------------------------- //
// fused forward + cross entropy
// --------------------------------------------------------------------------- //
// Workgroup = 8 waves = WC (class direction) x WS (sample direction).  The MFMA is
// issued "swapped" (A = W class tile, B = X sample tile) so that every lane owns ONE
// sample (column) and 16*CTW of its class logits (rows) in registers: the softmax
// reductions over classes are in-lane, then one half-swap, then WC values via LDS.
// FAST (host-checked: K % 16 == 0, 16-B aligned operands): every load is an unconditional 16-B
// vector load from a clamped address, so the compiler keeps counted vmcnt waits instead of
// branching around guarded loads (out-of-range rows load a valid row; their results are masked).
// MODE 0: guarded loads (any K / alignment).  MODE 1 ("FAST"): LDS-staged W and X chunks, unconditional 16-B loads.
// MODE 2 (round 3): W is NOT staged at all -- it streams global -> registers from a fragment-major fp32 shadow (see
// w_shadow32_kernel) through a 2-chunk register ring, the block's X rows are resident in LDS for a K-block of 64 KB, and the
// main loop has no barrier inside a K-block: with the 64-cycle fp32 MFMA the two waves of a SIMD keep the matrix pipe busy
// while their rings refill (the stream is 16 B/clk/CU, a quarter of what the bf16 forward pulls).  MODE 1 spent 28 % of its
// main loop between chunks (64 KB of W through registers into LDS and a barrier per 16 k: 5.67k cycles per chunk for 4.1k of
// MFMA; scripts/fwd32_stamps.py).  Same products in the same order as MODE 1: bit-identical results.
// LDS layout of fwd_ce_f32<CTW, WC, MODE> in floats: the kernel takes its offsets from it, the launcher its byte count.
template <int CTW, int WC, int MODE>
struct FwdLds {
    static constexpr int WS = 8 / WC, CPAD = 32 * CTW * WC, TS = 32 * WS;
    static constexpr int LDW = CPAD + 4, LDX = TS + 4;   // k-major rows of MODE 0's tiles
    // two LDS buffers of the (W, X) K-chunk ([KT][LDW] then [KT][LDX] each): chunk c+1 is written while chunk c feeds the MFMAs,
    // one barrier per chunk (the 64-cycle fp32 MFMAs of the partner wave cover the ds_write_b32 stream)
    static constexpr int BUF = KT * (LDW + LDX);
    static constexpr int STG = 8 * CTW * 32 * 32;        // epilogue: dZ staging, 8 waves x [CTW*32][32] floats (aliases the tile buffers)
    static constexpr int XK = 16384 / TS;                // MODE 2 / 3: K-block of the X rows resident in LDS: TS x XK floats = 64 KB
    static constexpr int XLD = XK + 4;                   // its row stride (floats): an odd multiple of 16 B -> the b128 reads of 16 rows hit 16 slots
    static constexpr int XT2 = MODE >= 2 ? TS * XLD : 0;
    static constexpr int TILE0 = 2 * BUF > STG ? 2 * BUF : STG;
    static constexpr int TILE = TILE0 > XT2 ? TILE0 : XT2;
    static constexpr int RED = TILE;                     // [WC][TS][4]
    static constexpr int RED2 = RED + WC * TS * 4;       // [WS][4]
    static constexpr size_t BYTES = sizeof(float) * (RED2 + WS * 4 + 16);
};

template <int CTW, int WC, int MODE>
__global__ __launch_bounds__(512) void fwd_ce_f32(FwdArgs a) {
    typedef FwdLds<CTW, WC, MODE> L;
    constexpr bool FAST = MODE >= 1;
    constexpr int WS = L::WS, CPAD = L::CPAD, TS = L::TS, LDW = L::LDW, LDX = L::LDX, BUF = L::BUF;
    constexpr int NPW = (CPAD * 4 + 511) / 512;     // float4 pieces of W per thread
    constexpr int NPX = (TS * 4 + 511) / 512;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Ws0 = smem;                    // [2][KT][LDW] then [KT][LDX]
    float* red = smem + L::RED;
    float* red2 = smem + L::RED2;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wc = wave % WC, ws = wave / WC;
    const int h = lane >> 5, l31 = lane & 31;
    const int sidx = (int)blockIdx.x >= a.seg[1].blk0 ? 1 : 0;
    const SegDesc& sg = a.seg[sidx];
    const int row0 = ((int)blockIdx.x - sg.blk0) * TS;
    const int C = a.C, K = a.K;
#define STAMP(i) do { if (a.stamps && lane == 0) a.stamps[((size_t)blockIdx.x * 8 + wave) * 8 + (i)] = __builtin_readcyclecounter(); } while (0)
    STAMP(0);
    const bool vecW = (K % 4 == 0) && ((reinterpret_cast<uintptr_t>(a.W) & 15) == 0);
    const bool vecX = (sg.ld % 4 == 0) && ((reinterpret_cast<uintptr_t>(sg.feats) & 15) == 0);

    // label of this lane's sample: dependent loads issued before the main loop hides them
    int lab_pre;
    {
        int rc = min(row0 + (wave / WC) * 32 + (lane & 31), sg.rows - 1);
        lab_pre = (int)sg.labels[sg.label_index ? sg.label_index[rc] : (int64_t)rc];
    }

    f32x16 acc[CTW];
#pragma unroll
    for (int ct = 0; ct < CTW; ++ct)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[ct][i] = 0.f;

    // A wave whose 32 sample rows all lie past the segment (batch 32 in a 64-row block: the reference's
    // own batch sizes are 8-64) or whose class tiles all lie past C skips its MFMAs: fp32 MFMA issue
    // (64 cycles per 32x32x2) is what bounds a single-workgroup forward, and its SIMD partner then
    // runs alone.  Wave-uniform; the accumulators stay 0 and the epilogue masks them as before.
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const bool wave_live = row0 + (wave_u / WC) * 32 < sg.rows && (wave_u % WC) * CTW * 32 < C;
    if constexpr (MODE >= 2) {
        // the streamed loops: the block's X rows are resident in LDS one K-block at a time, W streams into a register ring
        constexpr int XK = L::XK, XLD = L::XLD;
        constexpr int NPX2 = (TS * (XK / 4)) / 512;         // 16-B pieces of an X block per thread
        constexpr int PD = 2;                               // chunks (16 k) of W fragments in flight per wave
        float* Xt = smem;                                   // [TS][XLD]
        const float* xs2[NPX2];
#pragma unroll
        for (int q = 0; q < NPX2; ++q) {
            const int pp = tid + 512 * q;
            const int rc = min(row0 + pp / (XK / 4), sg.rows - 1);        // rows past the segment: coef = 0 below
            const int64_t rid = sg.feat_index ? sg.feat_index[rc] : (int64_t)rc;
            xs2[q] = sg.feats + (size_t)rid * sg.ld + 4 * (pp % (XK / 4));
        }
        auto x_stage = [&](int kb0, int kbw) {              // columns kb0 .. kb0 + kbw of the block's rows -> Xt, both barriers included
            f32x4v xr[NPX2];
#pragma unroll
            for (int q = 0; q < NPX2; ++q) {
                const int col = 4 * ((tid + 512 * q) % (XK / 4));
                xr[q] = *reinterpret_cast<const f32x4v*>(xs2[q] + kb0 + min(col, kbw - 4) - col);   // columns past the block: a valid piece nobody reads
            }
            __syncthreads();                                // previous block fully consumed
#pragma unroll
            for (int q = 0; q < NPX2; ++q) {
                const int pp = tid + 512 * q;
                *reinterpret_cast<f32x4v*>(Xt + (pp / (XK / 4)) * XLD + 4 * (pp % (XK / 4))) = xr[q];
            }
            __syncthreads();
        };
        const int nch = K / KT;                             // even (host-checked)
        if constexpr (MODE == 3) {
            // MODE 2's structure on the bf16 matrix pipe (umlh_f32_x3 in umlh_common.h): W arrives pre-split -- three bf16 piece planes
            // per fragment, [K/16 chunk][CPAD/32 tile][3 planes][64 lanes][8 bf16], 3 KB per (chunk, tile) instead of 2 KB --, the
            // wave splits its B fragment (8 floats of its sample row per chunk, read from the fp32 X block in LDS) in registers (44
            // VALU operations per chunk, issued under the MFMAs), and a chunk of a class tile is six v_mfma_f32_32x32x16_bf16
            // (192 cycles) instead of eight v_mfma_f32_32x32x2_f32 (512 cycles).  Same accumulator layout: the epilogue is shared.
            const u32x4s* wl = reinterpret_cast<const u32x4s*>(a.Ws) + (size_t)(wc * CTW) * 192 + lane;
            auto wfrag = [&](int c, int ct, int plane) -> u32x4s { return wl[((size_t)c * (CPAD / 32) + ct) * 192 + plane * 64]; };
            u32x4s ring[PD][CTW][3];
            if (wave_live) {
#pragma unroll
                for (int d = 0; d < PD; ++d)
#pragma unroll
                    for (int ct = 0; ct < CTW; ++ct)
#pragma unroll
                        for (int pl = 0; pl < 3; ++pl) ring[d][ct][pl] = wfrag(min(d, nch - 1), ct, pl);
            }
            STAMP(1);
            for (int kb0 = 0; kb0 < K; kb0 += XK) {
                const int kbw = min(XK, K - kb0);
                x_stage(kb0, kbw);
                if (wave_live) {
                    const int c0 = kb0 / KT, ncb = kbw / KT;
                    const float* xrow = Xt + (ws * 32 + l31) * XLD + 8 * h;
                    for (int c = 0; c < ncb; c += PD) {
#pragma unroll
                        for (int d = 0; d < PD; ++d) {
                            const f32x4v b0 = *reinterpret_cast<const f32x4v*>(xrow + (c + d) * KT);
                            const f32x4v b1 = *reinterpret_cast<const f32x4v*>(xrow + (c + d) * KT + 4);
                            u32x4s bp[3];
                            split3_into(bp, 0, b0[0], b0[1]);
                            split3_into(bp, 1, b0[2], b0[3]);
                            split3_into(bp, 2, b1[0], b1[1]);
                            split3_into(bp, 3, b1[2], b1[3]);
#pragma unroll
                            for (int ct = 0; ct < CTW; ++ct)
#pragma unroll
                                for (int pd = 0; pd < 6; ++pd)
                                    acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ring[d][ct][X3_ORDER[pd][0]]),
                                                                                      __builtin_bit_cast(bf16x8, bp[X3_ORDER[pd][1]]), acc[ct], 0, 0, 0);
                            const int nxt = min(c0 + c + d + PD, nch - 1);
#pragma unroll
                            for (int ct = 0; ct < CTW; ++ct)
#pragma unroll
                                for (int pl = 0; pl < 3; ++pl) ring[d][ct][pl] = wfrag(nxt, ct, pl);
                            // a tile's three planes are requested again as soon as its six MFMAs are out (not after the chunk's 24): more of
                            // the stream in flight per wave at the same register count
                            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);            // B reads
#pragma unroll
                            for (int ct = 0; ct < CTW; ++ct) {
                                __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);        // this tile's MFMAs (the split's VALU operations float between them)
                                __builtin_amdgcn_sched_group_barrier(0x020, 3, 0);        // its refill
                            }
                        }
                    }
                }
            }
        } else {
            // fragment (chunk c, class tile t): 64 lanes x 8 floats at Ws + ((c * CPAD/32 + t) * 64 + lane) * 8; lane (r, h) holds
            // W[32 t + r][16 c + 8 h .. + 8): the A operands of its eight 32x32x2 steps of the chunk (k order inside a chunk is
            // free as long as W and X agree; it is MODE 1's)
            const float* wl = a.Ws + ((size_t)(wc * CTW) * 64 + lane) * 8;
            auto wfrag = [&](int c, int ct, int half) -> f32x4v {
                return *reinterpret_cast<const f32x4v*>(wl + ((size_t)c * (CPAD / 32) + ct) * 512 + 4 * half);
            };
            f32x4v ring[PD][CTW][2];
            if (wave_live) {
#pragma unroll
                for (int d = 0; d < PD; ++d)
#pragma unroll
                    for (int ct = 0; ct < CTW; ++ct) { ring[d][ct][0] = wfrag(min(d, nch - 1), ct, 0); ring[d][ct][1] = wfrag(min(d, nch - 1), ct, 1); }
            }
            STAMP(1);
            for (int kb0 = 0; kb0 < K; kb0 += XK) {
                const int kbw = min(XK, K - kb0);               // multiple of 32
                x_stage(kb0, kbw);
                if (wave_live) {
                    const int c0 = kb0 / KT, ncb = kbw / KT;
                    const float* xrow = Xt + (ws * 32 + l31) * XLD + 8 * h;
                    for (int c = 0; c < ncb; c += PD) {
#pragma unroll
                        for (int d = 0; d < PD; ++d) {
                            const int cb = UMLH_ABL(a.dbg == 22 || a.dbg == 23) ? 0 : c + d;
                            const f32x4v b0 = *reinterpret_cast<const f32x4v*>(xrow + cb * KT);
                            const f32x4v b1 = *reinterpret_cast<const f32x4v*>(xrow + cb * KT + 4);
#pragma unroll
                            for (int s2 = 0; s2 < 8; ++s2)
#pragma unroll
                                for (int ct = 0; ct < CTW; ++ct)
                                    acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(ring[d][ct][s2 >> 2][s2 & 3], (s2 < 4 ? b0 : b1)[s2 & 3], acc[ct], 0, 0, 0);
                            const int nxt = UMLH_ABL(a.dbg == 21 || a.dbg == 23) ? 0 : min(c0 + c + d + PD, nch - 1);      // (past the end: a harmless re-load of the last chunk)
#pragma unroll
                            for (int ct = 0; ct < CTW; ++ct) { ring[d][ct][0] = wfrag(nxt, ct, 0); ring[d][ct][1] = wfrag(nxt, ct, 1); }
                            // pin the emitted order per chunk: B reads, its MFMAs, then the slot's refill loads (left alone, hipcc sinks
                            // every refill to the end of the loop body and the next iteration's first MFMA waits a full L2 round trip)
                            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);            // B reads
                            __builtin_amdgcn_sched_group_barrier(0x008, 8 * CTW, 0);      // MFMAs
                            __builtin_amdgcn_sched_group_barrier(0x020, 2 * CTW, 0);      // VMEM reads
                        }
                    }
                }
            }
        }
        __syncthreads();                                    // the epilogue's staging aliases the X block
    } else {
    // per-thread source rows (hoisted out of the K loop)
        const float* wsrc[NPW];
        const float* xsrc[NPX];
#pragma unroll
        for (int q = 0; q < NPW; ++q) {
            int p = tid + 512 * q, cls = p >> 2;
            if (FAST) wsrc[q] = a.W + (size_t)min(cls, C - 1) * K;        // rows >= C: logits masked to -inf below
            else wsrc[q] = (p < CPAD * 4 && cls < C) ? a.W + (size_t)cls * K : nullptr;
        }
#pragma unroll
        for (int q = 0; q < NPX; ++q) {
            int p = tid + 512 * q, smp = p >> 2, r = row0 + smp;
            const float* s = nullptr;
            if (FAST) {
                int rc = min(r, sg.rows - 1);                              // rows past the segment: coef = 0 below
                int64_t rid = sg.feat_index ? sg.feat_index[rc] : (int64_t)rc;
                s = sg.feats + (size_t)rid * sg.ld;
            } else if (p < TS * 4 && r < sg.rows) {
                int64_t rid = sg.feat_index ? sg.feat_index[r] : (int64_t)r;
                s = sg.feats + (size_t)rid * sg.ld;
            }
            xsrc[q] = s;
        }
    f32x4v wreg[NPW], xreg[NPX];
        auto gload = [&](int k0) {
#pragma unroll
            for (int q = 0; q < NPW; ++q) {
                int g = (tid + 512 * q) & 3;
                int k = k0 + 4 * g;
                if (FAST) wreg[q] = *reinterpret_cast<const f32x4v*>(wsrc[q] + k);
                else wreg[q] = wsrc[q] ? load4_guard(wsrc[q] + k, K - k, vecW) : f32x4v{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int q = 0; q < NPX; ++q) {
                int g = (tid + 512 * q) & 3;
                int k = k0 + 4 * g;
                if (FAST) xreg[q] = *reinterpret_cast<const f32x4v*>(xsrc[q] + k);
                else xreg[q] = xsrc[q] ? load4_guard(xsrc[q] + k, K - k, vecX) : f32x4v{0.f, 0.f, 0.f, 0.f};
            }
        };
        // FAST: the LDS tiles are [row][16 k] (row = class / sample, 64 B) with the four 16-B slots of a row XOR-swizzled by
        // (row >> 2) & 3: the 16-B pieces go to LDS as they come from memory (no transposing scalar stores), and the eight
        // k-steps of a chunk of one MFMA operand are two ds_read_b128 (lane half h multiplies k = 8h .. 8h+7; the order of k
        // inside a chunk is free as long as W and X agree) -- 10 LDS reads per 32 MFMAs instead of 40, 9 LDS stores per thread
        // instead of 36.  The swizzle makes both access patterns conflict-free without padding (same 64 KB per W buffer).
        auto lstore = [&](int buf) {
            float* Ws = Ws0 + buf * BUF;
            float* Xs = Ws + KT * LDW;
#pragma unroll
            for (int q = 0; q < NPW; ++q) {
                int p = tid + 512 * q;
                if (p < CPAD * 4) {
                    int cls = p >> 2, g = p & 3;
                    if (FAST) *reinterpret_cast<f32x4v*>(&Ws[cls * KT + 4 * (g ^ ((cls >> 2) & 3))]) = wreg[q];
                    else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) Ws[(4 * g + j) * LDW + cls] = wreg[q][j];
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < NPX; ++q) {
                int p = tid + 512 * q;
                if (p < TS * 4) {
                    int smp = p >> 2, g = p & 3;
                    if (FAST) *reinterpret_cast<f32x4v*>(&Xs[smp * KT + 4 * (g ^ ((smp >> 2) & 3))]) = xreg[q];
                    else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) Xs[(4 * g + j) * LDX + smp] = xreg[q][j];
                    }
                }
            }
        };
        auto compute = [&](int buf) {
            const float* Ws = Ws0 + buf * BUF;
            const float* Xs = Ws + KT * LDW;
            if (!wave_live) return;                       // ONE wave-uniform branch per chunk: the MFMA loop itself stays branch-free
            if (FAST) {
                const int sw = (l31 >> 2) & 3;            // tile bases are multiples of 32: (row >> 2) & 3 == (l31 >> 2) & 3
                const float* xr = Xs + (ws * 32 + l31) * KT;
                f32x4v b[2], av[CTW][2];
                b[0] = *reinterpret_cast<const f32x4v*>(xr + 4 * ((2 * h) ^ sw));
                b[1] = *reinterpret_cast<const f32x4v*>(xr + 4 * ((2 * h + 1) ^ sw));
#pragma unroll
                for (int ct = 0; ct < CTW; ++ct) {
                    const float* wr = Ws + ((wc * CTW + ct) * 32 + l31) * KT;
                    av[ct][0] = *reinterpret_cast<const f32x4v*>(wr + 4 * ((2 * h) ^ sw));
                    av[ct][1] = *reinterpret_cast<const f32x4v*>(wr + 4 * ((2 * h + 1) ^ sw));
                }
#pragma unroll
                for (int s2 = 0; s2 < 8; ++s2)
#pragma unroll
                    for (int ct = 0; ct < CTW; ++ct)
                        acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[ct][s2 >> 2][s2 & 3], b[s2 >> 2][s2 & 3], acc[ct], 0, 0, 0);
                return;
            }
#pragma unroll
            for (int kk = 0; kk < KT / 2; ++kk) {
                const int krow = 2 * kk + h;
                const float b = Xs[krow * LDX + ws * 32 + l31];
#pragma unroll
                for (int ct = 0; ct < CTW; ++ct) {
                    const float av = Ws[krow * LDW + (wc * CTW + ct) * 32 + l31];
                    acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b, acc[ct], 0, 0, 0);
                }
            }
        };

        // chunk c lives in buffer c & 1; registers hold chunk c+1 while chunk c is computed
        gload(0);
        lstore(0);
        if (FAST) gload(min(KT, K - KT)); else if (KT < K) gload(KT);
        __syncthreads();
        STAMP(1);
        int buf = 0;
        for (int k0 = 0; k0 < K; k0 += KT) {
            if (k0 + KT < K) lstore(buf ^ 1);                // chunk c+1 -> the other buffer (its readers passed the last barrier)
            if (FAST) gload(min(k0 + 2 * KT, K - KT));       // branch-free: tail prefetches re-load the last chunk
            else if (k0 + 2 * KT < K) gload(k0 + 2 * KT);
            compute(buf);
            __syncthreads();
            buf ^= 1;
        }

    }
    STAMP(2);
    // ---------------- epilogue: softmax cross entropy on the register tile ----------------
    // VALU-bound (16*CTW logits per lane, two waves per SIMD): round 3 rewrote it after the bf16 kernel's -- max by v_max3
    // chains, first arg-max by a descending equality scan with the register number as an inline constant, label logit by a
    // select tree on the bits of its register number, exp(u) as exp2(u * log2 e) on the exact u = fma(raw, scale, -max)
    // (the v_exp_f32 result is 1 ulp; the product's rounding is 6e-8 |u log2 e|, i.e. < 3e-6 relative on every term that is
    // not negligible against the max term: below the noise of the accumulation order, far below the 1e-4 this mode carries),
    // dZ staged through the (now free) LDS tile buffers and stored 16 B per lane = 8 class rows x 128 B per instruction
    // instead of 64 scattered 4-byte write-through stores per lane.  Padded classes (cls >= C) are handled in wave-uniform
    // branches that only the tile straddling C takes.
    const float scale = *sg.scale_ptr;
    const int smp = ws * 32 + l31;
    const int r = row0 + smp;
    const bool valid = r < sg.rows;
    const int lab = valid ? lab_pre : -1;
    constexpr int NREG = CTW * 16;
    const int wave_c0 = wc * CTW * 32;
    const float NEG_INF = -__builtin_huge_valf();
    const float LOG2E = 1.4426950408889634f;

    // z = raw * scale in place of raw is NOT kept (raw is needed for d loss / d scale): each pass forms it again (one multiply)
    float mx;
    int mi;
    {
        float mkc[CTW];
#pragma unroll
        for (int ct = 0; ct < CTW; ++ct) {
            const int cbase = wave_c0 + ct * 32;
            if (cbase + 32 > C) {                          // wave-uniform: the tile that straddles C (or lies past it)
                mkc[ct] = NEG_INF;
#pragma unroll
                for (int i = 0; i < 16; ++i) mkc[ct] = __builtin_fmaxf(mkc[ct], cbase + acc_row(i, h) < C ? acc[ct][i] * scale : NEG_INF);
            } else {
                mkc[ct] = acc[ct][0] * scale;
#pragma unroll
                for (int i = 1; i < 16; ++i) mkc[ct] = __builtin_fmaxf(mkc[ct], acc[ct][i] * scale);
            }
        }
        mx = mkc[0];
#pragma unroll
        for (int ct = 1; ct < CTW; ++ct) mx = __builtin_fmaxf(mx, mkc[ct]);
        // first register (= lowest class of this lane) that holds the lane's max
        int first = NREG;
#pragma unroll
        for (int ct = CTW - 1; ct >= 0; --ct) {
            const int cbase = wave_c0 + ct * 32;
            if (cbase + 32 > C) {
#pragma unroll
                for (int i = 15; i >= 0; --i) first = (cbase + acc_row(i, h) < C && acc[ct][i] * scale == mx) ? ct * 16 + i : first;
            } else {
#pragma unroll
                for (int i = 15; i >= 0; --i) first = acc[ct][i] * scale == mx ? ct * 16 + i : first;
            }
        }
        mi = first < NREG ? wave_c0 + (first >> 4) * 32 + (first & 3) + 8 * ((first >> 2) & 3) + 4 * h : 0x7fffffff;
    }
    {
        float omx = __shfl_xor(mx, 32);
        int omi = __shfl_xor(mi, 32);
        if (omx > mx || (omx == mx && omi < mi)) { mx = omx; mi = omi; }
    }
    if (WC > 1) {
        if (h == 0) { red[(wc * TS + smp) * 4 + 0] = mx; red[(wc * TS + smp) * 4 + 1] = __int_as_float(mi); }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < WC; ++w) {
            float omx = red[(w * TS + smp) * 4 + 0];
            int omi = __float_as_int(red[(w * TS + smp) * 4 + 1]);
            if (omx > mx || (omx == mx && omi < mi)) { mx = omx; mi = omi; }
        }
        __syncthreads();
    }
    STAMP(3);
    // label logit: register number = (tile, i) with i&3 = row&3, i>>2 = row>>3, h = (row>>2)&1
    const int rel = lab - wave_c0;
    const bool mine = rel >= 0 && rel < CTW * 32 && ((rel >> 2) & 1) == h;
    float rawy;
    {
        const int reg = (rel & 3) | ((rel >> 3) & 3) << 2 | (rel >> 5) << 4;
        float t[NREG];
#pragma unroll
        for (int ct = 0; ct < CTW; ++ct)
#pragma unroll
            for (int i = 0; i < 16; ++i) t[ct * 16 + i] = acc[ct][i];
#pragma unroll
        for (int bit = 0, n = NREG; n > 1; ++bit, n >>= 1) {
            const bool up = (reg >> bit) & 1;
#pragma unroll
            for (int j = 0; j < n / 2; ++j) t[j] = up ? t[2 * j + 1] : t[2 * j];
        }
        rawy = mine ? t[0] : 0.f;
    }
    const float rawy_lane = rawy;                           // this lane's own label logit (or 0)
    // e = exp(raw * scale - max), kept in the accumulators for the dZ pass
    float se = 0.f, serw = 0.f;
    const float nmx = -mx;
    const bool learn = a.learn != 0;
#pragma unroll
    for (int ct = 0; ct < CTW; ++ct) {
        const int cbase = wave_c0 + ct * 32;
        if (cbase + 32 > C) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float raw = acc[ct][i];
                const float e = cbase + acc_row(i, h) < C ? __builtin_amdgcn_exp2f(__builtin_fmaf(raw, scale, nmx) * LOG2E) : 0.f;
                se += e;
                serw = __builtin_fmaf(e, cbase + acc_row(i, h) < C ? raw : 0.f, serw);
                acc[ct][i] = e;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float raw = acc[ct][i];
                const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(raw, scale, nmx) * LOG2E);
                se += e;
                if (learn) serw = __builtin_fmaf(e, raw, serw);           // (wave-uniform: only learnable logit scales need it)
                acc[ct][i] = e;
            }
        }
    }
    float zy = rawy * scale;
    se += __shfl_xor(se, 32);
    serw += __shfl_xor(serw, 32);
    zy += __shfl_xor(zy, 32);
    rawy += __shfl_xor(rawy, 32);
    if (WC > 1) {
        if (h == 0) {
            float* d = red + (wc * TS + smp) * 4;
            d[0] = se; d[1] = serw; d[2] = zy; d[3] = rawy;
        }
        __syncthreads();
        se = serw = zy = rawy = 0.f;
#pragma unroll
        for (int w = 0; w < WC; ++w) {
            const float* d = red + (w * TS + smp) * 4;
            se += d[0]; serw += d[1]; zy += d[2]; rawy += d[3];
        }
    }
    STAMP(4);

    if (a.dzt != nullptr) {       // rows past the segment write zeros: the dW GEMM needs no masking of dZ^T
        const float coef = valid ? sg.w_over_rows * scale : 0.f;
        const float inv = 1.f / se;
        const float ic = inv * coef;                                  // one multiply per element (p * coef with p = e * inv differs in the last bit only)
        // every wave has passed the last barrier of the main loop (and the exchanges above): the tile buffers are free.
        // Wave-private staging tile [CTW*32 class rows][32 samples] fp32
        // (the slab tile idiom of slab_tile_stage / slab_tile_store, spelled out: through the helpers fwd_ce_f32<1,2,1> takes 66
        // VGPRs instead of 64 and loses a wave of occupancy)
        float* stg = smem + wave * (CTW * 32 * 32);
#pragma unroll
        for (int ct = 0; ct < CTW; ++ct)
#pragma unroll
            for (int i = 0; i < 16; ++i) stg[(ct * 32 + acc_row(i, h)) * 32 + l31] = acc[ct][i] * ic;
        if (mine) {                                          // the one-hot term, by the lane that owns the label's logit
            const float ey = __builtin_amdgcn_exp2f(__builtin_fmaf(rawy_lane, scale, nmx) * LOG2E);
            stg[rel * 32 + l31] = (ey * inv - 1.f) * coef;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float* dst = a.dzt + sg.col0 + row0 + ws * 32 + 4 * (lane & 7);
#pragma unroll
        for (int it = 0; it < CTW * 4; ++it) {
            const int row = it * 8 + (lane >> 3);
            const int cls = wave_c0 + row;
            const f32x4v v = *reinterpret_cast<const f32x4v*>(stg + row * 32 + 4 * (lane & 7));
            if (cls < C) store_out_f32x4(dst + (size_t)cls * a.ldz, v, a.plain);
        }
    }
    STAMP(5);

    // per-block sums of loss / top-1 / d(scale), taken once per sample (wc==0, h==0 lanes)
    float vl = 0.f, vc = 0.f, vg = 0.f;
    if (wc == 0 && h == 0 && valid) {
        vl = logf(se) + mx - zy;
        vc = (mi == lab) ? 1.f : 0.f;
        vg = serw / se - rawy;
        if (a.row_stats != nullptr) {
            float* rs = a.row_stats + 2 * ((size_t)(sidx ? a.seg[0].rows : 0) + r);
            rs[0] = vl;
            rs[1] = vc;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        vl += __shfl_xor(vl, off);
        vc += __shfl_xor(vc, off);
        vg += __shfl_xor(vg, off);
    }
    if (wc == 0 && lane == 0) { red2[ws * 4 + 0] = vl; red2[ws * 4 + 1] = vc; red2[ws * 4 + 2] = vg; }
    __syncthreads();
    if (tid == 0) {
        float l = 0.f, c = 0.f, g = 0.f;
#pragma unroll
        for (int w = 0; w < WS; ++w) { l += red2[w * 4 + 0]; c += red2[w * 4 + 1]; g += red2[w * 4 + 2]; }
        float* o = a.partials + (size_t)blockIdx.x * 4;
        o[0] = l; o[1] = c; o[2] = g; o[3] = 0.f;
    }
    STAMP(6);
#undef STAMP
}

// --------------------------------------------------------------------------- //
// generic GEMM  out[m][n] = alpha * sum_k A(m,k) B(n,k), 128x128 tile, 4 waves (2x2),
// each wave 64x64 = 2x2 MFMA tiles.  TA/TB = 0: operand stored with k contiguous
// (A[m*lda+k]);  = 1: stored k-major (A[k*lda+m]).  blockIdx.z = split-K slab.
// --------------------------------------------------------------------------- //
// tile = 64*TM x 64*TM, 4 waves (2x2) of TM x TM MFMA tiles each.  TM = 2 (128x128) maximises reuse; TM = 1
// (64x64) quadruples the workgroup count for GEMMs whose 128x128 grid cannot fill the chip.

// ---- split-K prologue shared by gemm_f32, dw_f32 and dw_f32x3 ----
// reduction rows per split whose row ids fit the LDS table (16 KB; 2048 sent cfg3's dW_head -- 2 splits of 4096 rows -- to the
// 64x64 gemm_f32 tile: 812 us instead of ~300)
constexpr int KIDS = 4096;

struct KRange { int kb, ke; };
// reduction range of split z: uniform chunks, or modality-aligned ones (GemmArgs::nsplit1)
__device__ __forceinline__ KRange splitk_range(const GemmArgs& g, int z) {
    int kb = z * g.k_chunk, ke = min(g.K, kb + g.k_chunk);
    if (g.nsplit1 > 0) {
        if (z < g.nsplit1) ke = min(g.k_switch, kb + g.k_chunk);
        else { kb = g.k_switch + (z - g.nsplit1) * g.k_chunk; ke = min(g.K, kb + g.k_chunk); }
    }
    return {kb, ke};
}

// reduction index k is a valid row of its modality (TB == 1: rows outside [0, k_valid) of either part are zeros)
__device__ __forceinline__ bool kvalid(const GemmArgs& g, int k) {
    return k < g.k_switch ? (k < g.k_valid1) : (k - g.k_switch < g.k_valid2);
}
// ... and lies inside the split; written with selects (the dW tiles evaluate it between MFMAs, without branches)
__device__ __forceinline__ bool kvalid_before(const GemmArgs& g, int k, int ke) {
    const bool first = k < g.k_switch;
    return (k < ke) & ((first ? k : k - g.k_switch) < (first ? g.k_valid1 : g.k_valid2));
}

// kid[i] = gathered row id of reduction row kb + i of this split, -1 = masked row; NT threads, ends with the barrier
template <int NT>
__device__ __forceinline__ void fill_row_ids(const GemmArgs& g, int* kid, int kb, int ke, int tid) {
    for (int i = tid; i < ke - kb; i += NT) {
        const int k = kb + i;
        int rid = -1;
        if (kvalid(g, k)) {
            if (k < g.k_switch) rid = g.k_rows ? (int)g.k_rows[k] : k;
            else { const int kl = k - g.k_switch; rid = g.k_rows2 ? (int)g.k_rows2[kl] : kl; }
        }
        kid[i] = rid;
    }
    __syncthreads();
}

// ---- slab tile store: a wave's NI x NJ accumulator tiles (32 x 32 each) -> its private LDS tile [32 NI rows][32 NJ columns] ->
// 16-byte row stores (a lane stores 16 B of one row instead of 64 scattered 4-byte write-through stores).  No padding: the
// ds_write_b32 of a register is 32 consecutive floats per lane half, and the ds_read_b128 of the rows of one store instruction
// is conflict-free in its 16-lane groups.  The LDS must be free (every wave past the main loop's last barrier). ----
template <int NI, int NJ>
__device__ __forceinline__ void slab_tile_stage(float* stg, const f32x16* acc, float mul, int lane) {
    const int h = lane >> 5, l31 = lane & 31;
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) stg[(i * 32 + acc_row(e, h)) * (32 * NJ) + j * 32 + l31] = acc[i * NJ + j][e] * mul;
}
// out: the tile's row 0 at this lane's column (4 * (lane % (8 NJ)) of the tile); tile row r is global row r0 + r, stored if < rlim
template <int NI, int NJ>
__device__ __forceinline__ void slab_tile_store(const float* stg, float* out, int ld, int r0, int rlim, bool col_ok, int plain, int lane) {
    constexpr int W = 32 * NJ, LPR = W / 4, RPI = 64 / LPR;      // floats per row, lanes per row, rows per store instruction
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int it = 0; it < 32 * NI / RPI; ++it) {
        const int row = it * RPI + lane / LPR;
        const f32x4v v = *reinterpret_cast<const f32x4v*>(stg + row * W + 4 * (lane % LPR));
        if (r0 + row < rlim && col_ok) store_out_f32x4(out + (size_t)(r0 + row) * ld, v, plain);
    }
}

template <int TA, int TB, int TM>
__global__ __launch_bounds__(256) void gemm_f32(GemmArgs g) {
    if (g.skip && *g.skip) return;
    constexpr int GBM = 64 * TM, GBN = 64 * TM, GLD = GBM + 4;
    // double-buffered K-chunks: one barrier per chunk, LDS writes of chunk c+1 overlap the MFMAs of chunk c
    __shared__ __attribute__((aligned(16))) float As2[2][KT * GLD];
    __shared__ __attribute__((aligned(16))) float Bs2[2][KT * GLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int h = lane >> 5, l31 = lane & 31;
    const int m0 = blockIdx.y * GBM, n0 = blockIdx.x * GBN;
    const KRange kr = splitk_range(g, blockIdx.z);
    const int kb = kr.kb, ke = kr.ke;

    f32x16 acc[TM][TM];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    f32x4v areg[TM], breg[TM];
    // ---- A ----  (GBM*4 16-B pieces per chunk = TM per thread)
    const float* a_src[TM];
    const bool vecA = (g.lda % 4 == 0) && ((reinterpret_cast<uintptr_t>(g.A) & 15) == 0);
    if (TA == 0) {
#pragma unroll
        for (int q = 0; q < TM; ++q) {
            int p = tid + 256 * q, row = p >> 2, m = m0 + row;
            const float* s = nullptr;
            if (m < g.M) {
                int64_t rid = g.a_rows ? g.a_rows[m] : (int64_t)m;
                s = g.A + (size_t)rid * g.lda;
            }
            a_src[q] = s;
        }
    }
    const bool vecB = (g.ldb % 4 == 0) && ((reinterpret_cast<uintptr_t>(g.B) & 15) == 0);
    const bool vecB2 = TB == 1 && g.B2 && (g.ldb2 % 4 == 0) && ((reinterpret_cast<uintptr_t>(g.B2) & 15) == 0);
    const float* b_src[TM];
    if (TB == 0) {
#pragma unroll
        for (int q = 0; q < TM; ++q) {
            int p = tid + 256 * q, row = p >> 2, n = n0 + row;
            b_src[q] = n < g.N ? g.B + (size_t)n * g.ldb : nullptr;
        }
    }
    // TB == 1: the gathered row id of every reduction row of this split is staged in LDS once.
    // Loading it per chunk made each chunk pay a dependent index->row round trip (~2 us x 64 chunks
    // on the cfg2 dW GEMM).  -1 = masked row.
    __shared__ int kid[KIDS];
    const bool use_kid = TB == 1 && (ke - kb) <= KIDS;
    if (use_kid) fill_row_ids<256>(g, kid, kb, ke, tid);

    auto gload = [&](int k0) {
#pragma unroll
        for (int q = 0; q < TM; ++q) {
            int p = tid + 256 * q;
            if (TA == 0) {                       // piece = (row m, 4 consecutive k)
                int k = k0 + 4 * (p & 3);
                f32x4v v = a_src[q] ? load4_guard(a_src[q] + k, ke - k, vecA) : f32x4v{0.f, 0.f, 0.f, 0.f};
                if (TB == 1) {                   // reduction index is a dZ^T column: mask padding
#pragma unroll
                    for (int j = 0; j < 4; ++j) if (!kvalid(g, k + j)) v[j] = 0.f;
                }
                areg[q] = v;
            } else {                             // piece = (k row, 4 consecutive m)
                int kk = p / (GBM / 4), mm = m0 + 4 * (p % (GBM / 4)), k = k0 + kk;
                areg[q] = (k < ke) ? load4_guard(g.A + (size_t)k * g.lda + mm, g.M - mm, vecA)
                                   : f32x4v{0.f, 0.f, 0.f, 0.f};
            }
            if (TB == 0) {
                int k = k0 + 4 * (p & 3);
                breg[q] = b_src[q] ? load4_guard(b_src[q] + k, ke - k, vecB) : f32x4v{0.f, 0.f, 0.f, 0.f};
            } else {
                int kk = p / (GBN / 4), nn = n0 + 4 * (p % (GBN / 4)), k = k0 + kk;
                f32x4v v = {0.f, 0.f, 0.f, 0.f};
                if (use_kid) {
                    int rid = k < ke ? kid[k - kb] : -1;
                    if (rid >= 0) {
                        const bool s2 = k >= g.k_switch;
                        v = load4_guard((s2 ? g.B2 : g.B) + (size_t)rid * (s2 ? g.ldb2 : g.ldb) + nn, g.N - nn, s2 ? vecB2 : vecB);
                    }
                } else if (k < ke && kvalid(g, k)) {
                    if (k < g.k_switch) {
                        int64_t rid = g.k_rows ? g.k_rows[k] : (int64_t)k;
                        v = load4_guard(g.B + (size_t)rid * g.ldb + nn, g.N - nn, vecB);
                    } else {
                        int kl = k - g.k_switch;
                        int64_t rid = g.k_rows2 ? g.k_rows2[kl] : (int64_t)kl;
                        v = load4_guard(g.B2 + (size_t)rid * g.ldb2 + nn, g.N - nn, vecB2);
                    }
                }
                breg[q] = v;
            }
        }
    };
    auto lstore = [&](int buf) {
        float* As = As2[buf];
        float* Bs = Bs2[buf];
#pragma unroll
        for (int q = 0; q < TM; ++q) {
            int p = tid + 256 * q;
            if (TA == 0) {
                int row = p >> 2, gq = p & 3;
#pragma unroll
                for (int j = 0; j < 4; ++j) As[(4 * gq + j) * GLD + row] = areg[q][j];
            } else {
                int kk = p / (GBM / 4), mm = 4 * (p % (GBM / 4));
                *reinterpret_cast<f32x4v*>(&As[kk * GLD + mm]) = areg[q];
            }
            if (TB == 0) {
                int row = p >> 2, gq = p & 3;
#pragma unroll
                for (int j = 0; j < 4; ++j) Bs[(4 * gq + j) * GLD + row] = breg[q][j];
            } else {
                int kk = p / (GBN / 4), nn = 4 * (p % (GBN / 4));
                *reinterpret_cast<f32x4v*>(&Bs[kk * GLD + nn]) = breg[q];
            }
        }
    };

    auto compute = [&](int buf) {
        const float* As = As2[buf];
        const float* Bs = Bs2[buf];
        if (TM == 2 && g.x3) {
            // products on the bf16 matrix pipe (umlh_f32_x3): lane half h takes k = 8h .. 8h+7 of the chunk in both operands (8 scalar
            // LDS reads per tile, as many as the fp32 form's), splits them three ways in registers and issues six
            // v_mfma_f32_32x32x16_bf16 per output tile (192 cycles) where the fp32 form issues eight 64-cycle MFMAs
            u32x4s fa[TM][3], fb[TM][3];
#pragma unroll
            for (int t = 0; t < TM; ++t) {
#pragma unroll
                for (int pr = 0; pr < 4; ++pr) {
                    split3_into(fa[t], pr, As[(8 * h + 2 * pr) * GLD + wm * 32 * TM + t * 32 + l31], As[(8 * h + 2 * pr + 1) * GLD + wm * 32 * TM + t * 32 + l31]);
                    split3_into(fb[t], pr, Bs[(8 * h + 2 * pr) * GLD + wn * 32 * TM + t * 32 + l31], Bs[(8 * h + 2 * pr + 1) * GLD + wn * 32 * TM + t * 32 + l31]);
                }
            }
#pragma unroll
            for (int pd = 0; pd < 6; ++pd)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TM; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[i][X3_ORDER[pd][0]]), __builtin_bit_cast(bf16x8, fb[j][X3_ORDER[pd][1]]), acc[i][j], 0, 0, 0);
            return;
        }
#pragma unroll
        for (int kk = 0; kk < KT / 2; ++kk) {
            const int krow = 2 * kk + h;
            float av[TM], bv[TM];
#pragma unroll
            for (int i = 0; i < TM; ++i) av[i] = As[krow * GLD + wm * 32 * TM + i * 32 + l31];
#pragma unroll
            for (int j = 0; j < TM; ++j) bv[j] = Bs[krow * GLD + wn * 32 * TM + j * 32 + l31];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TM; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
    };
    if (kb < ke) {
        gload(kb);
        lstore(0);
        if (kb + KT < ke) gload(kb + KT);
    }
    __syncthreads();
    int buf = 0;
    for (int k0 = kb; k0 < ke; k0 += KT) {
        if (k0 + KT < ke) lstore(buf ^ 1);               // chunk c+1 (in registers) -> the other buffer
        if (k0 + 2 * KT < ke) gload(k0 + 2 * KT);
        compute(buf);
        __syncthreads();
        buf ^= 1;
    }

    float* out = g.out + (size_t)blockIdx.z * g.slab_stride;
    const float alpha = g.alpha * (g.alpha_ptr ? *g.alpha_ptr : 1.f);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) {
            int n = n0 + wn * 32 * TM + j * 32 + l31;
            if (n >= g.N) continue;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                int m = m0 + wm * 32 * TM + i * 32 + acc_row(e, h);
                if (m < g.M) {
                    float v = acc[i][j][e] * alpha;
                    if (g.epi.on && gridDim.z == 1) v = epilogue_apply(g.epi, v, (long long)m * g.ldo + n, n);   // dense result: ldo == N
                    store_out_f32(out + (size_t)m * g.ldo + n, v, g.plain);
                }
            }
        }
}

// --------------------------------------------------------------------------- //
// dw_f32: dW = dZ^T F  (TA = 0, TB = 1 of gemm_f32's contract: A[m][k] k-contiguous, B rows gathered by reduction index,
// two sources, modality-aligned split-K) for the big-batch fp32 step.  128x128 tile, 4 waves of 64x64 (2x2 MFMA tiles).
// Against gemm_f32<0,1,1> (64x64 tiles, 114 us at cfg2): half the L2->CU bytes per flop, and the LDS tiles are
// [row][k] with a 20-float stride so that the 8 k-steps of a 16-row chunk of one MFMA operand are TWO ds_read_b128
// (lane half h takes k = 8h .. 8h+7 of the chunk -- the k order inside a chunk is free as long as A and B agree):
// 8 LDS reads per 32 MFMAs instead of 64 scalar ones.  All global loads are branch-free (clamped addresses; rows past
// M / columns past N only feed outputs that are never stored; masked reduction rows are zeroed by selects one
// iteration after the load was issued).
// --------------------------------------------------------------------------- //
constexpr int DWKC = 32;                                  // reduction rows per staged chunk (one 128-B line of a dZ^T row)
constexpr int DWLD = DWKC + 4;                            // floats per LDS row (b128 reads of 16 lanes cover all 64 banks)
constexpr size_t DW_SMEM = sizeof(float) * 4 * 128 * DWLD + sizeof(int) * KIDS;
__global__ __launch_bounds__(256) void dw_f32(GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) float dw_smem[];
    float* const As2 = dw_smem;                           // [2][128 * DWLD]
    float* const Bs2 = dw_smem + 2 * 128 * DWLD;          // [2][128 * DWLD]
    int* const kid = reinterpret_cast<int*>(dw_smem + 4 * 128 * DWLD);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, h = lane >> 5, l31 = lane & 31;
    // 1-D grid, split index fastest: workgroups are dealt to the 8 XCDs round-robin, so with 8 (or 16) splits every tile of
    // one K range runs on ONE XCD and its dZ^T columns / feature rows are fetched into that XCD's L2 once (with the tile
    // index fastest, the 4 column tiles sharing a dZ^T row block sat on 4 different XCDs)
    const int nsplit = (int)g.slab_count, z = blockIdx.x % nsplit, tile = blockIdx.x / nsplit, ntx = (g.N + 127) / 128;
    const int m0 = (tile / ntx) * 128, n0 = (tile % ntx) * 128;
    const KRange kr = splitk_range(g, z);
    const int kb = kr.kb, ke = kr.ke;
    fill_row_ids<256>(g, kid, kb, ke, tid);

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    // A pieces (4 per thread): row ar + 32q of the tile, k columns 4*akq .. +3 of the chunk (8 lanes = one 128-B line)
    const int ar = tid >> 3, akq = tid & 7;
    const float* a_row[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) a_row[q] = g.A + (size_t)min(m0 + ar + 32 * q, g.M - 1) * g.lda;
    // B pieces (4 per thread): reduction row bk of the chunk, columns 4*bnq + 32q .. +3 of the tile
    const int bk = tid & 31, bnq = tid >> 5;
    int b_col[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) b_col[q] = min(n0 + 4 * bnq + 32 * q, g.N - 4);
    f32x4v areg[4], breg[4];
    int a_k = 0;                                          // first reduction index of the staged A pieces (for the masks)
    bool b_ok = false;
    const float* b_row = g.B;
    auto gload_a = [&](int k0) {
        a_k = k0 + 4 * akq;
        const int kc = min(a_k, g.lda - 4);               // (only reduction indices >= K are ever clamped: masked below)
#pragma unroll
        for (int q = 0; q < 4; ++q) areg[q] = *reinterpret_cast<const f32x4v*>(a_row[q] + kc);
    };
    auto gload_b_row = [&](int k0) {
        const int k = k0 + bk;
        const int rid = kid[min(k, ke - 1) - kb];
        b_ok = (k < ke) & (rid >= 0);
        const bool s2 = k >= g.k_switch;
        const float* row = (s2 ? g.B2 : g.B) + (size_t)max(rid, 0) * (s2 ? g.ldb2 : g.ldb);
        b_row = b_ok ? row : g.B;
    };
    auto gload_b = [&]() {
#pragma unroll
        for (int q = 0; q < 4; ++q) breg[q] = *reinterpret_cast<const f32x4v*>(b_row + b_col[q]);
    };
    bool av[4];
    auto lstore_masks = [&]() {                           // validity of the 4 reduction indices of the staged A pieces (no branches)
#pragma unroll
        for (int j = 0; j < 4; ++j) av[j] = kvalid_before(g, a_k + j, ke);
    };
    auto lstore_piece = [&](int buf, int q) {
        float* As = As2 + buf * 128 * DWLD;
        float* Bs = Bs2 + buf * 128 * DWLD;
        f32x4v v = areg[q];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = av[j] ? v[j] : 0.f;
        *reinterpret_cast<f32x4v*>(&As[(ar + 32 * q) * DWLD + 4 * akq]) = v;
#pragma unroll
        for (int j = 0; j < 4; ++j) Bs[(4 * bnq + 32 * q + j) * DWLD + bk] = b_ok ? breg[q][j] : 0.f;
    };
    // One chunk = 64 MFMAs per wave (4096 cycles of the SIMD's matrix pipe) with ONE wave per SIMD: nothing else hides the
    // staging, and a block of ~150 staging instructions between two MFMA groups lets the pipe run dry (an MFMA occupies it
    // for 64 cycles = 16 issue slots).  So the LDS stores of chunk c+1 and the global loads of chunk c+2 are dealt out one
    // piece per MFMA step between the 16 steps of chunk c, the order pinned with sched_barrier.
    // Lane half h multiplies k = 16h .. 16h+15 of the chunk: 4 ds_read_b128 per operand tile.
    f32x4v a[2][4], b[2][4];
    auto mfma_step = [&](int s) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][s >> 2][s & 3], b[j][s >> 2][s & 3], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    };
    if (kb < ke) {
        gload_a(kb); gload_b_row(kb); gload_b();
        lstore_masks();
#pragma unroll
        for (int q = 0; q < 4; ++q) lstore_piece(0, q);
        if (kb + DWKC < ke) { gload_a(kb + DWKC); gload_b_row(kb + DWKC); gload_b(); }
    }
    __syncthreads();
    int buf = 0;
    for (int k0 = kb; k0 < ke; k0 += DWKC) {
        const float* As = As2 + buf * 128 * DWLD + (wm * 64 + l31) * DWLD + 16 * h;
        const float* Bs = Bs2 + buf * 128 * DWLD + (wn * 64 + l31) * DWLD + 16 * h;
        auto frag = [&](int v) {                          // operands of MFMA steps 4v .. 4v+3 (4 ds_read_b128)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i][v] = *reinterpret_cast<const f32x4v*>(As + i * 32 * DWLD + 4 * v);
                b[i][v] = *reinterpret_cast<const f32x4v*>(Bs + i * 32 * DWLD + 4 * v);
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        const bool st1 = k0 + DWKC < ke, ld2 = k0 + 2 * DWKC < ke;
        frag(0);
        frag(1);                                          // (the reads of steps 4v.. go out while steps 4(v-1).. multiply)
        mfma_step(0);
        if (st1) lstore_masks();
        __builtin_amdgcn_sched_barrier(0);
        mfma_step(1);
        frag(2);
#pragma unroll
        for (int q = 0; q < 4; ++q) {                     // chunk c+1 (in registers) -> the other buffer, a piece per step
            if (st1) lstore_piece(buf ^ 1, q);
            __builtin_amdgcn_sched_barrier(0);
            mfma_step(2 + q);
        }
        frag(3);
        if (ld2) gload_a(k0 + 2 * DWKC);
        __builtin_amdgcn_sched_barrier(0);
        mfma_step(6);
        if (ld2) gload_b_row(k0 + 2 * DWKC);
        __builtin_amdgcn_sched_barrier(0);
        mfma_step(7);
        mfma_step(8);
        if (ld2) gload_b();
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s2 = 9; s2 < 16; ++s2) mfma_step(s2);
        __syncthreads();
        buf ^= 1;
    }
    float* out = g.out + (size_t)z * g.slab_stride;
    const float alpha = g.alpha * (g.alpha_ptr ? *g.alpha_ptr : 1.f);
    // slab tile through the LDS tiles (free: every wave has passed the loop's last barrier), wave-private [64 rows][64 columns]:
    // 4 rows x 256 B per store instruction (the same change took 3 us off fwd_ce_f32)
    float* stg = dw_smem + wave * (64 * 64);
    slab_tile_stage<2, 2>(stg, &acc[0][0], alpha, lane);
    const int nq = n0 + wn * 64 + 4 * (lane & 15);
    slab_tile_store<2, 2>(stg, out + nq, g.ldo, m0 + wm * 64, g.M, nq < g.N, g.plain, lane);
}

// --------------------------------------------------------------------------- //
// dw_f32x3: dw_f32's product (same GemmArgs contract, same 128 x 128 tile, same split-K / modality rules) on the bf16 matrix
// pipe: fp32 operands split three ways, six piece products per product (umlh_f32_x3, umlh_common.h).
//   * EIGHT waves (2 x 4, 64 x 32 outputs each): with one wave per SIMD (dw_f32's four) the split's VALU work and the MFMAs of
//     the same wave did not overlap -- 352 VALU operations next to 48 MFMAs per chunk ran 84 -> 69 us, and splitting at staging
//     time, finer interleaving and a second register set for earlier prefetch (all built, all parity-clean) stayed at 60-67 us:
//     the sum of the two instruction streams, not their maximum.  Two waves per SIMD overlap them in hardware.
//   * the staging SPLITS: a thread splits the 16-byte pieces it has loaded (2 A pieces + 2 B pieces per chunk) and writes three
//     bf16 planes per operand -- every element is split once per workgroup, not once per wave that multiplies it.
//       A planes: [128 rows][32 k] bf16 = 64-byte rows, 16-byte slot s of row r stored at s ^ ((r >> 2) & 3): the b128 fragment
//                 reads (16-lane groups of rows {0-3, 12-15, 20-27} + 32i) and the 8-byte staging stores (16 lanes = 2 whole
//                 rows = all 32 store banks) are both conflict-free (an 80-byte padded row was for the reads only: 28 % of the
//                 LDS-active cycles were store conflicts, profiles/r03_fp32_x3_sq.txt); a lane's 16 k of the chunk are two
//                 groups of 8 = the k-slice of one v_mfma_f32_32x32x16_bf16 (lane half h holds k = 16h + 8g .. + 8 of group g)
//       B planes: [32 k][128 n] bf16 as the rows arrive (no transposing scalar stores); a thread holds 8 consecutive columns of
//                 its k-row and stores 16 bytes per plane; 16-byte chunk ch of k-row r is stored at
//                 ch ^ (((r & 3) << 2) | ((r >> 1) & 1) | (((r >> 2) & 1) << 1)): eight consecutive rows of one chunk hit eight
//                 different 16-byte bank groups (b128 stores), and the ds_read_b64_tr_b16 fragments (4 k-rows x 16 columns per
//                 16-lane group) stay conflict-free as in dw_bf16
//   * per chunk (32 k) and wave: 2 groups x (6 A reads + 6 B reads) and 2 x 12 MFMAs; chunk c+1 is staged from registers while
//     chunk c multiplies, chunk c+2 is requested right after -- a barrier per chunk.
// --------------------------------------------------------------------------- //
constexpr int X3_ARS = 64, X3_APL = 128 * X3_ARS, X3_BPL = 32 * 256, X3_BUF = 3 * X3_APL + 3 * X3_BPL;   // bytes per A row / A plane / B plane / buffer
constexpr size_t DW_SMEM_X3 = 2 * (size_t)X3_BUF + sizeof(int) * KIDS;
__global__ __launch_bounds__(512) void dw_f32x3(GemmArgs g) {
    typedef unsigned int u32x2s __attribute__((ext_vector_type(2)));
    typedef short s16x4 __attribute__((ext_vector_type(4)));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    extern __shared__ __attribute__((aligned(16))) float dw_smem[];
    unsigned char* const lds = reinterpret_cast<unsigned char*>(dw_smem);
    int* const kid = reinterpret_cast<int*>(lds + 2 * X3_BUF);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 2, wn = wave & 3, h = lane >> 5, l31 = lane & 31;
    const int g16 = lane >> 4, q4 = (lane & 15) >> 2, p4 = lane & 3;
    const int nsplit = (int)g.slab_count, z = blockIdx.x % nsplit, tile = blockIdx.x / nsplit, ntx = (g.N + 127) / 128;
    const int m0 = (tile / ntx) * 128, n0 = (tile % ntx) * 128;
    const KRange kr = splitk_range(g, z);
    const int kb = kr.kb, ke = kr.ke;
    fill_row_ids<512>(g, kid, kb, ke, tid);

    f32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;

    // A pieces (2 per thread): row ar + 64q of the tile, k columns 4*akq .. +3 of the chunk; B pieces (2 per thread): reduction
    // row bk of the chunk, columns 8*bnq + 4q .. +3 of the tile (8 consecutive columns per thread)
    const int ar = tid >> 3, akq = tid & 7;
    const int bk = tid & 31, bnq = tid >> 5;
    const float* a_row[2];
    int b_col[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        a_row[q] = g.A + (size_t)min(m0 + ar + 64 * q, g.M - 1) * g.lda;
        b_col[q] = min(n0 + 8 * bnq + 4 * q, g.N - 4);
    }
    f32x4v areg[2], breg[2];
    int a_k = 0;
    bool b_ok = false;
    bool chunk_full = false;                              // every reduction row of the chunk in the registers is valid: no masks (uniform)
    auto gload = [&](int k0) {
        a_k = k0 + 4 * akq;
        {   // rows k0 .. k0 + 31 all valid?  (one modality, inside its valid count and inside the split)
            const bool first = k0 < g.k_switch;
            const int last = k0 + DWKC - 1;
            chunk_full = last < ke && (first ? (last < g.k_switch && last < g.k_valid1) : (last - g.k_switch < g.k_valid2));
        }
        const int kc = min(a_k, g.lda - 4);               // (only reduction indices >= K are ever clamped: masked below)
#pragma unroll
        for (int q = 0; q < 2; ++q) areg[q] = *reinterpret_cast<const f32x4v*>(a_row[q] + kc);
        const int k = k0 + bk;
        const int rid = kid[min(k, ke - 1) - kb];
        b_ok = (k < ke) & (rid >= 0);
        const bool s2 = k >= g.k_switch;
        const float* row = (s2 ? g.B2 : g.B) + (size_t)max(rid, 0) * (s2 ? g.ldb2 : g.ldb);
        const float* br = b_ok ? row : g.B;
#pragma unroll
        for (int q = 0; q < 2; ++q) breg[q] = *reinterpret_cast<const f32x4v*>(br + b_col[q]);
    };
    const int a_wr = ar * X3_ARS + ((((akq >> 1) ^ (ar >> 2)) & 3) << 4) + 8 * (akq & 1);   // + 64 q * X3_ARS  (row + 64: same swizzle)
    const int b_sw = ((bk & 3) << 2) | ((bk >> 1) & 1) | (((bk >> 2) & 1) << 1);
    const int b_wr = 3 * X3_APL + bk * 256 + ((bnq ^ b_sw) << 4);
    auto stage = [&](int buf) {                           // split the four pieces in registers, three planes each
        unsigned char* base = lds + buf * X3_BUF;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            f32x4v v = areg[q];
            if (!chunk_full) {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = kvalid_before(g, a_k + j, ke) ? v[j] : 0.f;
            }
            const Split3 s0 = split3_pair(v[0], v[1]), s1 = split3_pair(v[2], v[3]);
            unsigned char* d = base + a_wr + 64 * q * X3_ARS;
            *reinterpret_cast<u32x2s*>(d) = u32x2s{s0.hi, s1.hi};
            *reinterpret_cast<u32x2s*>(d + X3_APL) = u32x2s{s0.mid, s1.mid};
            *reinterpret_cast<u32x2s*>(d + 2 * X3_APL) = u32x2s{s0.lo, s1.lo};
        }
        {
            f32x4v v0 = breg[0], v1 = breg[1];
            if (!chunk_full) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { v0[j] = b_ok ? v0[j] : 0.f; v1[j] = b_ok ? v1[j] : 0.f; }
            }
            const Split3 s0 = split3_pair(v0[0], v0[1]), s1 = split3_pair(v0[2], v0[3]), s2 = split3_pair(v1[0], v1[1]), s3 = split3_pair(v1[2], v1[3]);
            unsigned char* d = base + b_wr;
            *reinterpret_cast<u32x4s*>(d) = u32x4s{s0.hi, s1.hi, s2.hi, s3.hi};
            *reinterpret_cast<u32x4s*>(d + X3_BPL) = u32x4s{s0.mid, s1.mid, s2.mid, s3.mid};
            *reinterpret_cast<u32x4s*>(d + 2 * X3_BPL) = u32x4s{s0.lo, s1.lo, s2.lo, s3.lo};
        }
    };
    // fragment addresses
    const int a_rd = (wm * 64 + l31) * X3_ARS;                                // + i * 32 * X3_ARS + (slot ^ a_sw) * 16 + plane * X3_APL,  slot = 2h + g
    const int a_sw = (l31 >> 2) & 3;                                         // ((row >> 2) & 3: the tile bases are multiples of 32)
    const int b_ch = wn * 4 + (g16 & 1) * 2 + (p4 >> 1);                     // 16-byte chunk of this lane's 4 columns
    const int b_rd = 3 * X3_APL + (16 * h + q4) * 256 + 8 * (p4 & 1);         // + (8 g + 4 hi) * 256 + (chunk ^ swizzle) * 16 + plane * X3_BPL
    if (kb < ke) {
        gload(kb);
        stage(0);
        if (kb + DWKC < ke) gload(kb + DWKC);
    }
    __syncthreads();
    int buf = 0;
    for (int k0 = kb; k0 < ke; k0 += DWKC) {
        const unsigned char* base = lds + buf * X3_BUF;
        const bool st1 = k0 + DWKC < ke, ld2 = k0 + 2 * DWKC < ke;
#pragma unroll
        for (int g2 = 0; g2 < 2; ++g2) {
            bf16x8 A[2][3], B[3];
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
                for (int i = 0; i < 2; ++i) A[i][pl] = *reinterpret_cast<const bf16x8*>(base + pl * X3_APL + a_rd + i * 32 * X3_ARS + (((2 * h + g2) ^ a_sw) << 4));
                const unsigned char* r0 = base + pl * X3_BPL + b_rd + 8 * g2 * 256;
                // swizzle of k-row r = 16h + 8g + 4hi + q4:  ((r & 3) << 2) | ((r >> 1) & 1) | (((r >> 2) & 1) << 1)  =  (q4 << 2) | (q4 >> 1) | (hi << 1)
                const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(r0 + ((b_ch ^ ((q4 << 2) | (q4 >> 1))) << 4)));
                const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(r0 + 4 * 256 + ((b_ch ^ ((q4 << 2) | (q4 >> 1) | 2)) << 4)));
                const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                B[pl] = __builtin_bit_cast(bf16x8, v);
            }
#pragma unroll
            for (int pd = 0; pd < 6; ++pd)
#pragma unroll
                for (int i = 0; i < 2; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[i][X3_ORDER[pd][0]], B[X3_ORDER[pd][1]], acc[i], 0, 0, 0);
            if (g2 == 0) {
                if (st1) stage(buf ^ 1);                  // chunk c+1 (in registers) -> the other buffer, under the MFMAs above and the partner wave's
                if (ld2) gload(k0 + 2 * DWKC);            // ... and the registers are free for chunk c+2: a whole chunk of time to land
            }
            // (running the two waves of a SIMD in opposite phase -- one staging while the other multiplies -- was measured: 137-144 us
            // per step against 119 with every wave in this order)
        }
        __syncthreads();
        buf ^= 1;
    }
    float* out = g.out + (size_t)z * g.slab_stride;
    const float alpha = g.alpha * (g.alpha_ptr ? *g.alpha_ptr : 1.f);
    // slab tile through the (free) LDS, wave-private [64 rows][32 columns]: a lane stores 16 B of one row
    float* stg = dw_smem + wave * (64 * 32);
    slab_tile_stage<2, 1>(stg, acc, alpha, lane);
    const int nq = n0 + wn * 32 + 4 * (lane & 7);
    slab_tile_store<2, 1>(stg, out + nq, g.ldo, m0 + wm * 64, g.M, nq < g.N, g.plain, lane);
}

// --------------------------------------------------------------------------- //
// gemm_enc: the dense layers of the MultiBench encoder (no row gathers).  Same contract as gemm_f32 with a 64x64 tile,
// but the K range is staged 64 reduction rows at a time and the NEXT 64 are already in flight while a chunk is multiplied:
// these GEMMs are short (K = 40 .. 300, or a split-K range of 64-128 rows of a 1600 / 2048 long reduction) and tiny, so
// their duration is the chain of dependent memory round trips, not MFMA time (20-32 MFMAs per chunk).  gemm_f32 walks K in
// 16-row chunks with one barrier and one round trip each: 3 round trips for K = 40, 5 for an 80-row split.
// --------------------------------------------------------------------------- //
constexpr int EKC = 64;
#ifdef UMLH_ABLATIONS
__device__ unsigned long long* g_gemm_stamps = nullptr;   // analysis build: 16 cycle stamps of block (0,0,0) thread 0 (UMLH_DBG_GEMM_STAMPS = device address)
#endif
template <int TA, int TB>
__global__ __launch_bounds__(256) void gemm_enc(GemmArgs g) {
    constexpr int LDA_ = TA == 0 ? 65 : 68, LDB_ = TB == 0 ? 65 : 68;   // transposing scalar stores want an odd stride, b128 stores 16-B rows
    __shared__ __attribute__((aligned(16))) float As[EKC * LDA_];
    __shared__ __attribute__((aligned(16))) float Bs[EKC * LDB_];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, h = lane >> 5, l31 = lane & 31;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const int kb = blockIdx.z * g.k_chunk, ke = min(g.K, kb + g.k_chunk);
    // 16-B pieces are loaded without branches (a guarded load per piece puts every load in its own basic block and the
    // compiler waits for each before issuing the next: 8 dependent round trips per chunk): a piece is whole or absent --
    // guaranteed when the contiguous extent is a multiple of 4 -- and an absent piece reads the operand's first 16 bytes
    // and is zeroed by a select.  Operands that do not qualify (lda = 35, unaligned base) take 4 clamped scalar loads.
    const bool vecA = (g.lda % 4 == 0) && ((reinterpret_cast<uintptr_t>(g.A) & 15) == 0) && ((TA == 0 ? g.K : g.M) % 4 == 0);
    const bool vecB = (g.ldb % 4 == 0) && ((reinterpret_cast<uintptr_t>(g.B) & 15) == 0) && ((TB == 0 ? g.K : g.N) % 4 == 0);
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    f32x4v areg[4], breg[4];
    const int pr = tid >> 4, pq = tid & 15;              // piece q of the thread: row/k-row pr + 16q, 16-B column pq
    // piece at base[row*ld + col .. col+3]; row_ok: the row exists; lim: valid elements from col (<= 0: none)
    auto piece = [&](const float* base, size_t row, int ld, int col, bool row_ok, int lim, bool vec) -> f32x4v {
        f32x4v v;
        if (vec) {
            const bool ok = row_ok && lim >= 4;
            v = *reinterpret_cast<const f32x4v*>(ok ? base + row * ld + col : base);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = ok ? v[j] : 0.f;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool ok = row_ok && j < lim;
                const float x = *(ok ? base + row * ld + col + j : base);
                v[j] = ok ? x : 0.f;
            }
        }
        return v;
    };
    auto gload = [&](int k0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = pr + 16 * q;
            if (TA == 0) areg[q] = piece(g.A, (size_t)(m0 + r), g.lda, k0 + 4 * pq, m0 + r < g.M, ke - (k0 + 4 * pq), vecA);       // A[m][k]
            else         areg[q] = piece(g.A, (size_t)(k0 + r), g.lda, m0 + 4 * pq, k0 + r < ke, g.M - (m0 + 4 * pq), vecA);       // A[k][m]
            if (TB == 0) breg[q] = piece(g.B, (size_t)(n0 + r), g.ldb, k0 + 4 * pq, n0 + r < g.N, ke - (k0 + 4 * pq), vecB);
            else         breg[q] = piece(g.B, (size_t)(k0 + r), g.ldb, n0 + 4 * pq, k0 + r < ke, g.N - (n0 + 4 * pq), vecB);
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = pr + 16 * q;
            if (TA == 0) {
#pragma unroll
                for (int j = 0; j < 4; ++j) As[(4 * pq + j) * LDA_ + r] = areg[q][j];
            } else *reinterpret_cast<f32x4v*>(&As[r * LDA_ + 4 * pq]) = areg[q];
            if (TB == 0) {
#pragma unroll
                for (int j = 0; j < 4; ++j) Bs[(4 * pq + j) * LDB_ + r] = breg[q][j];
            } else *reinterpret_cast<f32x4v*>(&Bs[r * LDB_ + 4 * pq]) = breg[q];
        }
    };
#ifdef UMLH_ABLATIONS
    unsigned long long* stp = (g_gemm_stamps && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && tid == 0) ? g_gemm_stamps : nullptr;
    int sti = 0;
#define GSTAMP() do { if (stp && sti < 15) stp[sti++] = __builtin_readcyclecounter(); } while (0)
#else
#define GSTAMP() do { } while (0)
#endif
    GSTAMP();
    if (kb < ke) gload(kb);
    GSTAMP();
    for (int k0 = kb; k0 < ke; k0 += EKC) {
        lstore();
        GSTAMP();
        __syncthreads();
        GSTAMP();
        if (k0 + EKC < ke) gload(k0 + EKC);
        const int steps = (min(EKC, ke - k0) + 1) >> 1;  // rows past ke hold zeros
        const float* ap = As + h * LDA_ + wm * 32 + l31;
        const float* bp = Bs + h * LDB_ + wn * 32 + l31;
#pragma unroll 4
        for (int kk = 0; kk < steps; ++kk)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * kk * LDA_], bp[2 * kk * LDB_], acc, 0, 0, 0);
        GSTAMP();
        if (k0 + EKC < ke) __syncthreads();
    }
    float* out = g.out + (size_t)blockIdx.z * g.slab_stride;
    const int n = n0 + wn * 32 + l31;
    if (n < g.N) {
        if (!(g.epi.on && gridDim.z == 1)) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + wm * 32 + acc_row(e, h);
                if (m < g.M) out[(size_t)m * g.ldo + n] = acc[e] * g.alpha;
            }
        } else {
            // the operand loads of the tail are hoisted and batched (16 independent loads in flight); element by element
            // behind `if (bias) .. if (gate) ..` they cost one memory round trip each (~9k of this kernel's ~20k cycles)
            const Epilogue ep = g.epi;
            const float bias = ep.bias ? ep.bias[n] : 0.f;
            const unsigned long long seed = ep.seed + (ep.seed_ptr ? *ep.seed_ptr : 0ull);
            float gt[16], ad[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) { gt[e] = 1.f; ad[e] = 0.f; }
            if (ep.gate) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int m = m0 + wm * 32 + acc_row(e, h);
                    gt[e] = ep.gate[m < g.M ? (size_t)m * g.ldo + n : (size_t)n];
                }
            }
            if (ep.add) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int m = m0 + wm * 32 + acc_row(e, h);
                    ad[e] = ep.add[m < g.M ? (size_t)m * g.ldo + n : (size_t)n];
                }
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + wm * 32 + acc_row(e, h);
                float v = acc[e] * g.alpha + bias;
                if (ep.relu) v = fmaxf(v, 0.f);
                v = gt[e] > 0.f ? v : 0.f;
                if (ep.thresh) v = keep_elem(seed, (unsigned long long)((long long)m * g.ldo + n), ep.thresh) ? v * ep.inv_keep : 0.f;
                v += ad[e];
                if (m < g.M) out[(size_t)m * g.ldo + n] = v;
            }
        }
    }
    GSTAMP();
#ifdef UMLH_ABLATIONS
    if (stp) stp[15] = (unsigned long long)sti;
#endif
}

// --------------------------------------------------------------------------- //
// slab reduction (+ optimizer update)
// --------------------------------------------------------------------------- //
// MODE 0: grad_out = sum of slabs.  MODE 1: p,m,v updated from the sum (grad_out
// optional).  n = number of parameters (multiple of 4 not required).
template <int MODE>
__global__ __launch_bounds__(256) void reduce_update(const float* __restrict__ slabs, int n_slabs,
                                                     long long slab_stride, long long n,
                                                     float* __restrict__ grad_out, float* __restrict__ p,
                                                     float* __restrict__ m, float* __restrict__ v, OptArgs o,
                                                     long long frozen_lo, long long frozen_hi) {
    long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    // elements [frozen_lo, frozen_hi) (multiples of 4) keep their value and moments: the constant row of an img_proj with bias
    if (MODE == 1 && i >= frozen_lo && i < frozen_hi) return;
    if (i + 4 <= n && (slab_stride % 4 == 0)) {
        f32x4v gsum = {0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < n_slabs; ++s)
            gsum += *reinterpret_cast<const f32x4v*>(slabs + (size_t)s * slab_stride + i);
        if (grad_out) store_out_f32x4(grad_out + i, gsum, o.plain);
        if (MODE == 1) {
            f32x4v pp = *reinterpret_cast<f32x4v*>(p + i);
            f32x4v mm = *reinterpret_cast<f32x4v*>(m + i);
            f32x4v vv = {0.f, 0.f, 0.f, 0.f};
            if (o.kind != UMLH_OPT_SGD) vv = *reinterpret_cast<f32x4v*>(v + i);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float a = pp[j], b = mm[j], c = vv[j];
                opt_update(o, gsum[j], a, b, c);
                pp[j] = a; mm[j] = b; vv[j] = c;
            }
            store_out_f32x4(p + i, pp, o.plain);
            store_out_f32x4(m + i, mm, o.plain);
            if (o.kind != UMLH_OPT_SGD) store_out_f32x4(v + i, vv, o.plain);
        }
    } else {
        for (long long e = i; e < n && e < i + 4; ++e) {
            float gs = 0.f;
            for (int s = 0; s < n_slabs; ++s) gs += slabs[(size_t)s * slab_stride + e];
            if (grad_out) grad_out[e] = gs;
            if (MODE == 1) {
                float a = p[e], b = m[e], c = (o.kind != UMLH_OPT_SGD) ? v[e] : 0.f;
                opt_update(o, gs, a, b, c);
                p[e] = a; m[e] = b;
                if (o.kind != UMLH_OPT_SGD) v[e] = c;
            }
        }
    }
}

// --------------------------------------------------------------------------- //
// optimizer.step() over many parameter tensors in one launch: workgroup b works on tensor t with blk0[t] <= b < blk0[t+1]
// --------------------------------------------------------------------------- //
struct MultiOptArgs {
    float* p[UMLH_MULTI_OPT_MAX]; const float* g[UMLH_MULTI_OPT_MAX]; float* m[UMLH_MULTI_OPT_MAX]; float* v[UMLH_MULTI_OPT_MAX];
    long long n[UMLH_MULTI_OPT_MAX];
    int blk0[UMLH_MULTI_OPT_MAX + 1];
    int n_tensors;
};

__global__ __launch_bounds__(256) void multi_opt_kernel(MultiOptArgs a, OptArgs o) {
    int t = 0;
    for (int i = 1; i < a.n_tensors; ++i) t = (int)blockIdx.x >= a.blk0[i] ? i : t;
    const long long i0 = ((long long)((int)blockIdx.x - a.blk0[t]) * 256 + threadIdx.x) * 4;
    const long long n = a.n[t];
    float* p = a.p[t]; const float* g = a.g[t]; float* m = a.m[t]; float* v = a.v[t];
    for (long long e = i0; e < n && e < i0 + 4; ++e) {
        float pp = p[e], mm = m[e], vv = o.kind != UMLH_OPT_SGD ? v[e] : 0.f;
        opt_update(o, g[e], pp, mm, vv);
        p[e] = pp; m[e] = mm;
        if (o.kind != UMLH_OPT_SGD) v[e] = vv;
    }
}

// --------------------------------------------------------------------------- //
// per-step scalars + logit-scale parameters
// --------------------------------------------------------------------------- //
__global__ __launch_bounds__(256) void finalize_kernel(FinalizeArgs f) {
    __shared__ float sh[6][256];
    finalize_body<false>(f, sh);
}

// --------------------------------------------------------------------------- //
// head step: ONE launch for everything after the dW GEMM of a training step --
// sum the split-K slabs, apply the optimizer to (W, m, v), refresh the bf16 fragment-major
// shadow of W that the next forward streams (bf16 mode), and (last block) reduce the forward
// partials to the step's scalars + update the learnable logit scales.
// --------------------------------------------------------------------------- //
// 4 consecutive elements per thread (twice the workgroups of an 8-element split: at C*d = 512 000 that is 500 workgroups
// = 2 per CU instead of one 4-wave workgroup per CU, and the kernel is bound by bytes in flight, not by arithmetic).
__global__ __launch_bounds__(256) void head_step_kernel(const float* __restrict__ slabs, int n_slabs, long long slab_stride,
                                                        int C, int K, float* __restrict__ p, float* __restrict__ m,
                                                        float* __restrict__ v, OptArgs o, unsigned short* __restrict__ shadow,
                                                        int cpad, FinalizeArgs f, float* __restrict__ grad_out, DiagArgs dg,
                                                        float* __restrict__ shadow32) {
    __shared__ float sh[6][256];
    if (blockIdx.x == gridDim.x - 1) { finalize_body<false>(f, sh); return; }
    const long long g4 = (long long)blockIdx.x * 256 + threadIdx.x;      // group of 4 consecutive k of one class row
    const long long n4 = (long long)C * K / 4;
    const bool live = g4 < n4;
    const long long i = (live ? g4 : 0) * 4;
    // image slabs and text slabs are summed separately (the split-K is modality-aligned): their
    // dot product / norms / sign agreement are the reference's per-step gradient diagnostics
    f32x4v gi = {0.f, 0.f, 0.f, 0.f}, gt = gi;
    f32x4v p0 = gi, m0 = gi, v0 = gi;
    const bool upd = live && grad_out == nullptr;
    if (upd) {                                               // issued before the slab sums: more bytes in flight per thread
        p0 = *reinterpret_cast<f32x4v*>(p + i);
        m0 = *reinterpret_cast<f32x4v*>(m + i);
        if (o.kind != UMLH_OPT_SGD) v0 = *reinterpret_cast<f32x4v*>(v + i);
    }
    if (live) {
        for (int s = 0; s < dg.n_slabs_img; ++s) gi += *reinterpret_cast<const f32x4v*>(slabs + (size_t)s * slab_stride + i);
        for (int s = dg.n_slabs_img; s < n_slabs; ++s) gt += *reinterpret_cast<const f32x4v*>(slabs + (size_t)s * slab_stride + i);
    }
    if (dg.dst != nullptr) {                                 // uniform over the grid
        float dot = 0.f, n2i = 0.f, n2t = 0.f, agree = 0.f;
        if (live) {
            const int col0 = dg.cols > 0 ? (int)(i % K) : 0;   // (K is a multiple of 4: the four elements share a class row)
            const int lim = dg.cols > 0 ? dg.cols : 0x7fffffff;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool in = col0 + j < lim;
                const float a = in ? gi[j] * dg.inv_w0 : 0.f;
                const float b = in ? gt[j] * dg.inv_w1 : 0.f;
                dot = __builtin_fmaf(a, b, dot);
                n2i = __builtin_fmaf(a, a, n2i);
                n2t = __builtin_fmaf(b, b, n2t);
                const int sa = (a > 0.f) - (a < 0.f), sb = (b > 0.f) - (b < 0.f);
                agree += in && sa == sb ? 1.f : 0.f;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            dot += __shfl_xor(dot, off); n2i += __shfl_xor(n2i, off);
            n2t += __shfl_xor(n2t, off); agree += __shfl_xor(agree, off);
        }
        const int w = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) { sh[0][w] = dot; sh[1][w] = n2i; sh[2][w] = n2t; sh[3][w] = agree; }
        __syncthreads();
        const int nblk = (int)gridDim.x - 1;                 // (the last block of the grid is the finalize block)
        if (threadIdx.x < 4) {
            const float t = sh[threadIdx.x][0] + sh[threadIdx.x][1] + sh[threadIdx.x][2] + sh[threadIdx.x][3];
            __hip_atomic_store(dg.part + (size_t)blockIdx.x * 4 + threadIdx.x, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __threadfence();
        }
        __syncthreads();
        if (threadIdx.x == 0)
            sh[4][0] = __hip_atomic_fetch_add(dg.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(nblk - 1) ? 1.f : 0.f;
        __syncthreads();
        if (sh[4][0] != 0.f) {                               // last ticket: every workgroup's partials are published
            const int q = threadIdx.x >> 6, l = threadIdx.x & 63;
            float t = 0.f;
            for (int b = l; b < nblk; b += 64) t += __hip_atomic_load(dg.part + (size_t)b * 4 + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off);
            if (l == 0) dg.dst[q] = t;
            if (threadIdx.x == 0) __hip_atomic_store(dg.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (!live) return;
    const f32x4v g0 = gi + gt;
    if (grad_out != nullptr) {             // data-parallel split: gradient only, the update follows the all-reduce
        store_out_f32x4(grad_out + i, g0, o.plain);
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float a = p0[j], b = m0[j], c = v0[j];
        opt_update(o, g0[j], a, b, c);
        p0[j] = a; m0[j] = b; v0[j] = c;
    }
    store_out_f32x4(p + i, p0, o.plain);
    store_out_f32x4(m + i, m0, o.plain);
    if (o.kind != UMLH_OPT_SGD) store_out_f32x4(v + i, v0, o.plain);
    if (shadow != nullptr) {
        const int cls = (int)(i / K), k = (int)(i % K);
        const long long piece = ((long long)(k >> 4) * (cpad / 32) + (cls >> 5)) * 64 + (cls & 31) + 32 * ((k >> 3) & 1);
        typedef unsigned int u32x2s __attribute__((ext_vector_type(2)));
        const u32x2s w = {pack_bf16x2(p0[0], p0[1]), pack_bf16x2(p0[2], p0[3])};
        if (o.plain) *reinterpret_cast<u32x2s*>(shadow + piece * 8 + (k & 7)) = w;
        else asm volatile("global_store_dwordx2 %0, %1, off sc1" ::"v"(shadow + piece * 8 + (k & 7)), "v"(w) : "memory");
    }
    if (shadow32 != nullptr && o.x3) {     // three-plane bf16 split of the new weights (w_shadow_x3_kernel's layout): 4 values = half a lane slot per plane
        const int cls = (int)(i / K), k = (int)(i % K);
        typedef unsigned int u32x2s __attribute__((ext_vector_type(2)));
        u32x2s hi, mid, lo;
        { const Split3 s3 = split3_pair(p0[0], p0[1]); hi[0] = s3.hi; mid[0] = s3.mid; lo[0] = s3.lo; }
        { const Split3 s3 = split3_pair(p0[2], p0[3]); hi[1] = s3.hi; mid[1] = s3.mid; lo[1] = s3.lo; }
        unsigned short* base = reinterpret_cast<unsigned short*>(shadow32) +
                               (((long long)(k >> 4) * (cpad / 32) + (cls >> 5)) * 192 + (cls & 31) + 32 * ((k >> 3) & 1)) * 8 + (k & 7);
        if (o.plain) {
            *reinterpret_cast<u32x2s*>(base) = hi; *reinterpret_cast<u32x2s*>(base + 512) = mid; *reinterpret_cast<u32x2s*>(base + 1024) = lo;
        } else {
            asm volatile("global_store_dwordx2 %0, %1, off sc1" ::"v"(base), "v"(hi) : "memory");
            asm volatile("global_store_dwordx2 %0, %1, off sc1" ::"v"(base + 512), "v"(mid) : "memory");
            asm volatile("global_store_dwordx2 %0, %1, off sc1" ::"v"(base + 1024), "v"(lo) : "memory");
        }
    } else if (shadow32 != nullptr) {      // fp32 fragment-major shadow of the new weights (w_shadow32_kernel's layout): 4 floats = half a lane slot
        const int cls = (int)(i / K), k = (int)(i % K);
        const long long piece = ((long long)(k >> 4) * (cpad / 32) + (cls >> 5)) * 64 + (cls & 31) + 32 * ((k >> 3) & 1);
        store_out_f32x4(shadow32 + piece * 8 + (k & 7), p0, o.plain);
    }
}

// --------------------------------------------------------------------------- //
// zero-shot head init: one block per class, rows accumulated in index order.  The labels are scanned 256 at a time
// (every thread looking at ALL n labels cost 2.8 ms at ImageNet's 29 940 text rows); the matches of a window are
// compacted in row order (wave ballot + prefix), so each column still adds its rows in ascending order -- the
// result is bit-identical to the serial scan.
// --------------------------------------------------------------------------- //
__global__ __launch_bounds__(256) void zero_shot_kernel(const float* __restrict__ feats,
                                                        const int64_t* __restrict__ labels, long long n, int d,
                                                        float* __restrict__ w) {
    extern __shared__ float zsum[];          // [d] + [256]
    __shared__ int midx[256];
    __shared__ int wcnt[4];
    float* redn = zsum + d;
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int j = tid; j < d; j += 256) zsum[j] = 0.f;            // column j is owned by thread j % 256 throughout
    int count = 0;
    for (long long base = 0; base < n; base += 256) {
        const long long r = base + tid;
        const bool hit = r < n && labels[r] == c;
        const unsigned long long bal = __ballot(hit);
        if (lane == 0) wcnt[wv] = __popcll(bal);
        __syncthreads();
        int off = 0;
        for (int k = 0; k < wv; ++k) off += wcnt[k];
        const int total = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        if (hit) midx[off + __popcll(bal & ((1ULL << lane) - 1ULL))] = tid;
        __syncthreads();
        for (int q = 0; q < total; ++q) {
            const float* row = feats + (size_t)(base + midx[q]) * d;
            for (int j = tid; j < d; j += 256) zsum[j] += row[j];
        }
        count += total;
        __syncthreads();                                          // midx / wcnt are rewritten by the next window
    }
    float ss = 0.f;
    for (int j = tid; j < d; j += 256) {
        float mean = count > 0 ? zsum[j] / (float)count : 0.f;
        zsum[j] = mean;
        ss += mean * mean;
    }
    redn[tid] = ss;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) redn[tid] += redn[tid + off];
        __syncthreads();
    }
    float nrm = fmaxf(sqrtf(redn[0]), 1e-12f);
    for (int j = tid; j < d; j += 256) w[(size_t)c * d + j] = zsum[j] / nrm;
}

// --------------------------------------------------------------------------- //
// epoch shuffles without a sort: out[i] = pi(i), the Feistel permutation of umlh_feistel.h.
// Used for throughput-mode loaders (order_rng="device"); reference-identical orders come from
// the CPU sampler restatement instead.
// --------------------------------------------------------------------------- //
__global__ __launch_bounds__(256) void feistel_perm_kernel(long long n, unsigned long long seed, int half,
                                                           long long* __restrict__ out) {
    long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = feistel_index(i, n, seed, half);
}

// --------------------------------------------------------------------------- //
// the row ids of a block of steps: every span of both modalities in one launch, one thread per id.  A span owns the 256-id
// blocks blk0 .. blk0 + ceil(count / 256) - 1; a block finds its span by walking the (at most 32) descriptors, which is
// uniform over the block.  FEISTEL ids are computed in place (no permutation of n rows is written), TABLE ids are copied.
// --------------------------------------------------------------------------- //
__global__ __launch_bounds__(256) void index_block_kernel(IndexBlockArgs a) {
    int s = 0;
    while (s + 1 < a.count && (int)blockIdx.x >= a.s[s + 1].blk0) ++s;
    const IndexSpanDesc& d = a.s[s];
    const long long j = (long long)((int)blockIdx.x - d.blk0) * 256 + threadIdx.x;
    if (j >= d.count) return;
    const long long i = d.start + j;
    long long id = i;
    if (d.kind == UMLH_SPAN_FEISTEL) id = feistel_index(i, d.n, d.seed, d.half);
    else if (d.kind == UMLH_SPAN_TABLE) id = d.order[i];
    d.dst[j] = id;
}

// --------------------------------------------------------------------------- //
// fp32 head-weight shadow for fwd_ce_f32 MODE 2, MFMA-FRAGMENT-MAJOR: [K/16 chunk][CPAD/32 class tile][64 lanes][8 floats];
// lane l = (r, h) of tile t, chunk c holds W[32 t + r][16 c + 8 h .. + 8): a wave fetches the A operands of a chunk of one
// class tile with two fully coalesced 1-KiB loads straight into registers.  Class rows >= C are zero.  One thread per 16 B.
// --------------------------------------------------------------------------- //
__global__ __launch_bounds__(256) void w_shadow32_kernel(const float* __restrict__ w, float* __restrict__ dst, int C, int K, int cpad) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    const int tiles = cpad / 32;
    const long long total = (long long)(K / 16) * tiles * 128;
    if (q >= total) return;
    const int half = (int)(q & 1), lane = (int)((q >> 1) & 63);
    const int tile = (int)((q >> 7) % tiles), c = (int)((q >> 7) / tiles);
    const int cls = tile * 32 + (lane & 31);
    f32x4v v = {0.f, 0.f, 0.f, 0.f};
    if (cls < C) v = *reinterpret_cast<const f32x4v*>(w + (size_t)cls * K + c * 16 + 8 * (lane >> 5) + 4 * half);
    *reinterpret_cast<f32x4v*>(dst + q * 4) = v;
}

// The same fragments as three bf16 piece planes (umlh_f32_x3, umlh_common.h): [K/16 chunk][CPAD/32 tile][plane][64 lanes][8 bf16];
// one thread per half lane slot (4 values).
__global__ __launch_bounds__(256) void w_shadow_x3_kernel(const float* __restrict__ w, unsigned short* __restrict__ dst, int C, int K, int cpad) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    const int tiles = cpad / 32;
    const long long total = (long long)(K / 16) * tiles * 128;
    if (q >= total) return;
    const int half = (int)(q & 1), lane = (int)((q >> 1) & 63);
    const int tile = (int)((q >> 7) % tiles), c = (int)((q >> 7) / tiles);
    const int cls = tile * 32 + (lane & 31);
    f32x4v v = {0.f, 0.f, 0.f, 0.f};
    if (cls < C) v = *reinterpret_cast<const f32x4v*>(w + (size_t)cls * K + c * 16 + 8 * (lane >> 5) + 4 * half);
    typedef unsigned int u32x2s __attribute__((ext_vector_type(2)));
    u32x2s hi, mid, lo;
    { const Split3 s3 = split3_pair(v[0], v[1]); hi[0] = s3.hi; mid[0] = s3.mid; lo[0] = s3.lo; }
    { const Split3 s3 = split3_pair(v[2], v[3]); hi[1] = s3.hi; mid[1] = s3.mid; lo[1] = s3.lo; }
    unsigned short* base = dst + (((long long)c * tiles + tile) * 192 + lane) * 8 + 4 * half;
    *reinterpret_cast<u32x2s*>(base) = hi;
    *reinterpret_cast<u32x2s*>(base + 512) = mid;
    *reinterpret_cast<u32x2s*>(base + 1024) = lo;
}

// --------------------------------------------------------------------------- //
// launchers (called from umlh_api.cpp)
// --------------------------------------------------------------------------- //
extern "C" {

int umlh_launch_w_shadow32(const float* w, float* dst, int C, int K, int cpad, hipStream_t stream) {
    if (K % 16 != 0 || cpad % 32 != 0) return (int)hipErrorInvalidValue;
    const long long total = (long long)(K / 16) * (cpad / 32) * 128;
    if (umlh_f32_x3()) {       // (dst holds 1.5x the fp32 shadow's bytes: umlh_api.cpp Layout::w32s)
        hipLaunchKernelGGL(w_shadow_x3_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, w, (unsigned short*)dst, C, K, cpad);
        return (int)hipGetLastError();
    }
    hipLaunchKernelGGL(w_shadow32_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, w, dst, C, K, cpad);
    return (int)hipGetLastError();
}

// fwd_ce configuration for a class count: WC waves along classes, CTW 32-class
// tiles per wave.  Returns samples per block (TS) or 0 if C is unsupported.
int umlh_f32_fwd_config(int C, int* ctw, int* wc) {
    if (C < 1 || C > 1024) return 0;
    int tiles = (C + 31) / 32;
    int w = 1;
    while (w < tiles && w < 8) w *= 2;
    int t = (tiles + w - 1) / w;
    if (t == 3) t = 4;
    *ctw = t; *wc = w;
    return 32 * (8 / w);
}

#define FWD_CASE_F(CT, W, F)                                                                        \
    if (ctw == CT && wc == W && mode == F) {                                                        \
        size_t sm = FwdLds<CT, W, F>::BYTES;                                                        \
        if (int e = raise_lds_limit<&fwd_ce_f32<CT, W, F>>((int)sm)) return e;                      \
        FwdArgs c_ = *a; c_.plain = umlh_plain_stores();                                            \
        hipLaunchKernelGGL((fwd_ce_f32<CT, W, F>), dim3(grid), dim3(512), sm, stream, c_);          \
        return (int)hipGetLastError();                                                              \
    }
#define FWD_CASE(CT, W) FWD_CASE_F(CT, W, 3) FWD_CASE_F(CT, W, 2) FWD_CASE_F(CT, W, 1) FWD_CASE_F(CT, W, 0)

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int umlh_f32_launch_fwd(const FwdArgs* a, int ctw, int wc, int grid, hipStream_t stream) {
    if (grid <= 0) return 0;
    bool fast = a->K % KT == 0 && aligned16(a->W);
    for (int s = 0; s < 2; ++s)
        if (a->seg[s].rows > 0) fast = fast && a->seg[s].ld % 4 == 0 && aligned16(a->seg[s].feats);
    // MODE 2 (W streamed from the fragment-major shadow): the caller keeps the shadow current (umlh_launch_w_shadow32 /
    // the update kernel) and passes it in a->Ws; UMLH_F32_FWD=1 keeps the LDS-staged kernel for A/B timing
    static const bool no_stream = env_int("UMLH_F32_FWD", 0) == 1;
    const int mode = !fast ? 0 : ((a->Ws != nullptr && a->K % (2 * KT) == 0 && !no_stream) ? (a->x3 ? 3 : 2) : 1);
    FWD_CASE(1, 1) FWD_CASE(1, 2) FWD_CASE(1, 4) FWD_CASE(1, 8) FWD_CASE(2, 8) FWD_CASE(4, 8)
    return (int)hipErrorInvalidValue;
}

static bool dw_f32_applies(const GemmArgs* g, int ta, int tb) {
    static const bool off = env_int("UMLH_F32_DW", 1) == 0;   // timing comparisons
    if (off || ta != 0 || tb != 1 || g->a_rows || g->epi.on || g->skip) return false;
    if ((long long)g->M * g->N < 8LL * 128 * 128 || g->N < 4 || g->N % 4 || g->lda < 4) return false;
    if (g->k_chunk > KIDS) return false;
    if (g->lda % 4 || g->ldb % 4 || (reinterpret_cast<uintptr_t>(g->A) & 15) || (reinterpret_cast<uintptr_t>(g->B) & 15)) return false;
    if (g->ldo % 4 || g->slab_stride % 4 || (reinterpret_cast<uintptr_t>(g->out) & 15)) return false;      // 16-byte slab stores
    if (g->B2 && (g->ldb2 % 4 || (reinterpret_cast<uintptr_t>(g->B2) & 15))) return false;
    if (!g->B2 && g->k_switch < g->K) return false;
    return true;
}

int umlh_f32_launch_gemm(const GemmArgs* g, int ta, int tb, int splits, hipStream_t stream) {
    if (g->M <= 0 || g->N <= 0) return 0;
    if (dw_f32_applies(g, ta, tb)) {
        if (int e = raise_lds_limit<&dw_f32>((int)DW_SMEM)) return e;
        if (int e = raise_lds_limit<&dw_f32x3>((int)DW_SMEM_X3)) return e;
        GemmArgs a = *g;
        a.slab_count = splits;
        a.plain = umlh_plain_stores();
        if (umlh_f32_x3()) hipLaunchKernelGGL(dw_f32x3, dim3(((g->N + 127) / 128) * ((g->M + 127) / 128) * splits), dim3(512), DW_SMEM_X3, stream, a);
        else hipLaunchKernelGGL(dw_f32, dim3(((g->N + 127) / 128) * ((g->M + 127) / 128) * splits), dim3(256), DW_SMEM, stream, a);
        return (int)hipGetLastError();
    }
    // 64x64 tiles when the 128x128 grid would leave most of the 256 CUs with a single 4-wave workgroup
    long long wg128 = (long long)((g->N + 127) / 128) * ((g->M + 127) / 128) * splits;
    static const int tm_env = env_int("UMLH_F32_TM", 0);   // tile override for tuning runs
    const int tm = (tm_env == 1 || tm_env == 2) ? tm_env : (wg128 < 768 ? 1 : 2);
    const int t = 64 * tm;
    dim3 grid((g->N + t - 1) / t, (g->M + t - 1) / t, splits);
    GemmArgs c = *g;
    c.plain = umlh_plain_stores();
    c.x3 = (tm == 2 && umlh_f32_x3()) ? 1 : 0;
#define GEMM_CASE(A_, B_, T_) if (ta == A_ && tb == B_ && tm == T_) { hipLaunchKernelGGL((gemm_f32<A_, B_, T_>), grid, dim3(256), 0, stream, c); return (int)hipGetLastError(); }
    GEMM_CASE(0, 0, 1) GEMM_CASE(0, 0, 2) GEMM_CASE(0, 1, 1) GEMM_CASE(0, 1, 2) GEMM_CASE(1, 1, 1) GEMM_CASE(1, 1, 2)
    return (int)hipErrorInvalidValue;
}

int umlh_f32_launch_gemm_enc(const GemmArgs* g, int ta, int tb, int splits, hipStream_t stream) {
    if (g->M <= 0 || g->N <= 0) return 0;
    if (g->a_rows || g->k_rows || g->B2 || g->nsplit1 || g->alpha_ptr) return (int)hipErrorInvalidValue;
    dim3 grid((g->N + 63) / 64, (g->M + 63) / 64, splits);
#ifdef UMLH_ABLATIONS
    {
        const char* e = getenv("UMLH_DBG_GEMM_STAMPS");
        static int last_sel = -2;
        static int call = 0;
        unsigned long long* ptr = (e && env_int("UMLH_DBG_GEMM_CALL", -1) == call)   /* index of the gemm_enc launch to stamp */ ? (unsigned long long*)strtoull(e, nullptr, 0) : nullptr;
        (void)last_sel;
        ++call;
        hipMemcpyToSymbolAsync(HIP_SYMBOL(g_gemm_stamps), &ptr, sizeof(ptr), 0, hipMemcpyHostToDevice, stream);
    }
#endif
#define GEMM_ENC_CASE(A_, B_) if (ta == A_ && tb == B_) { hipLaunchKernelGGL((gemm_enc<A_, B_>), grid, dim3(256), 0, stream, *g); return (int)hipGetLastError(); }
    GEMM_ENC_CASE(0, 0) GEMM_ENC_CASE(0, 1) GEMM_ENC_CASE(1, 1)
    return (int)hipErrorInvalidValue;
}

int umlh_launch_reduce_update(int mode, const float* slabs, int n_slabs, long long slab_stride, long long n,
                              float* grad_out, float* p, float* m, float* v, const OptArgs* o, long long frozen_lo,
                              long long frozen_hi, hipStream_t stream) {
    if (n <= 0) return 0;
    if (frozen_lo < frozen_hi && (frozen_lo % 4 || frozen_hi % 4)) return (int)hipErrorInvalidValue;
    int blocks = (int)((n + 1023) / 1024);
    if (mode == 0)
        hipLaunchKernelGGL((reduce_update<0>), dim3(blocks), dim3(256), 0, stream, slabs, n_slabs, slab_stride, n,
                           grad_out, p, m, v, *o, frozen_lo, frozen_hi);
    else
        hipLaunchKernelGGL((reduce_update<1>), dim3(blocks), dim3(256), 0, stream, slabs, n_slabs, slab_stride, n,
                           grad_out, p, m, v, *o, frozen_lo, frozen_hi);
    return (int)hipGetLastError();
}

int umlh_launch_multi_opt(int n, float* const* p, const float* const* g, float* const* m, float* const* v, const long long* cnt,
                          const OptArgs* o, hipStream_t stream) {
    MultiOptArgs a;
    a.n_tensors = n;
    int blocks = 0;
    for (int i = 0; i < n; ++i) {
        a.p[i] = p[i]; a.g[i] = g[i]; a.m[i] = m[i]; a.v[i] = v ? v[i] : nullptr; a.n[i] = cnt[i];
        a.blk0[i] = blocks;
        blocks += (int)((cnt[i] + 1023) / 1024);
    }
    a.blk0[n] = blocks;
    if (blocks == 0) return 0;
    hipLaunchKernelGGL(multi_opt_kernel, dim3(blocks), dim3(256), 0, stream, a, *o);
    return (int)hipGetLastError();
}

// hf: the slabs, the head (or grad_out) and the optimizer / finalize arguments, as make_head_fuse fills them (n_sub, dw_per_row
// and n_slabs_img belong to the one-launch step: the slab order of this launch is dg's)
int umlh_launch_head_step(const HeadFuse* hf, const DiagArgs* dg, float* shadow32, hipStream_t stream) {
    long long n4 = (long long)hf->C * hf->K / 4;
    int blocks = (int)((n4 + 255) / 256) + 1;                 // + the finalize block
    DiagArgs d = *dg;
    if (d.dst && (!d.part || !d.ticket)) return (int)hipErrorInvalidValue;
    if (d.n_slabs_img > hf->n_slabs) d.n_slabs_img = hf->n_slabs;
    OptArgs oc = hf->o;
    oc.plain = umlh_plain_stores();
    oc.x3 = umlh_f32_x3();
    hipLaunchKernelGGL(head_step_kernel, dim3(blocks), dim3(256), 0, stream, hf->slabs, hf->n_slabs, hf->slab_stride, hf->C, hf->K,
                       hf->p, hf->m, hf->v, oc, hf->shadow, hf->cpad, hf->f, hf->grad_out, d, shadow32);
    return (int)hipGetLastError();
}

int umlh_launch_feistel_perm(long long n, unsigned long long seed, long long* out, hipStream_t stream) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(feistel_perm_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, seed, feistel_half(n), out);
    return (int)hipGetLastError();
}

// a->s[i].half and .blk0 are filled here; spans with count == 0 are legal (they own no block)
int umlh_launch_index_block(IndexBlockArgs* a, hipStream_t stream) {
    long long blocks = 0;
    for (int i = 0; i < a->count; ++i) {
        IndexSpanDesc& d = a->s[i];
        d.half = d.kind == UMLH_SPAN_FEISTEL ? feistel_half(d.n) : 0;
        d.blk0 = (int)blocks;
        blocks += (d.count + 255) / 256;
        if (blocks > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    }
    if (blocks == 0) return 0;
    hipLaunchKernelGGL(index_block_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, *a);
    return (int)hipGetLastError();
}

int umlh_launch_finalize(const FinalizeArgs* f, hipStream_t stream) {
    hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(256), 0, stream, *f);
    return (int)hipGetLastError();
}

int umlh_launch_zero_shot(const float* feats, const int64_t* labels, long long n, int d, int C, float* w,
                          hipStream_t stream) {
    size_t sm = sizeof(float) * (size_t)(d + 256);
    hipLaunchKernelGGL(zero_shot_kernel, dim3(C), dim3(256), sm, stream, feats, labels, n, d, w);
    return (int)hipGetLastError();
}

}  // extern "C"
