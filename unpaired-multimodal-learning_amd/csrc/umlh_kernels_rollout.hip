// The autoregressive rollout of the MultiBench model (reference: MultiBench/train.py:268-292) and the spectral-bias spectra
// (train.py:245-251) for gfx950.
//
// rollout_rows.  Every rollout step is an encoder forward at T = 1, where the causal softmax over one key is exactly 1:
// attention is out_proj(v_proj(h)), no row sees another row, and the whole chain of one row is
//     cur_0 = x0[r];  for s = 1..steps:
//       h = Wc (W_in cur_{s-1} + b_in) + pos0                       (Wc, pos0 optional)
//       per layer: a = W_o (W_v h + b_v) + b_o;  h = LN1(h + a);  f = W_2 relu(W_1 h + b_1) + b_2;  h = LN2(h + f)
//       cur_s = W_out h + b_out;   out[r, s, :] = cur_s  (s = 0: the seed)
// One launch walks all steps.  A workgroup of 512 threads (8 waves) owns 16 rows and never reads what another workgroup
// writes and never waits for one: any grid size is safe.  Activations live in LDS, weights are read from global memory
// (they are the same for every workgroup and every step: L2 / Infinity Cache traffic).
//
//   products      v_mfma_f32_16x16x4_f32: the A operand is a 16-output-column x 4-k piece of a weight matrix (one 16-byte
//                 load of four adjacent k per lane), the B operand 4 k x the 16 rows of the workgroup.  A wave owns the
//                 output tiles wave, wave + 8, ... (at most four at a time, independent accumulators) and walks K in blocks
//                 of 16: MFMA i of a block takes k = k0 + i, k0 + 4 + i, k0 + 8 + i, k0 + 12 + i, blocks ascending -- one
//                 fp32 fma chain per output in an order that depends on K alone.  Out-of-range k and columns are zeros.
//   LDS layout    an activation [K][16 rows] is stored as [K / 4][16][4]: the B operand of a block is one conflict-free
//                 ds_read_b128 per lane, and the accumulator of an output tile (4 adjacent columns x 1 row per lane) is one
//                 ds_write_b128 at the place the next product reads it.  Producers write whole 16-column tiles with zeros
//                 past the width, which is what the next product's K padding needs.
//   FFN           the hidden block is produced 512 columns at a time up to Z = 128, 256 above (32 / 16 KiB), and consumed at
//                 once by the second product, whose accumulators stay in registers across the chunks (Z <= 512: four tiles
//                 per wave).
//   narrow N      a product with fewer output tiles than waves (z = 40: 3) splits its reduction across the idle waves in
//                 contiguous runs of blocks; the partial sums meet in LDS and are added in run order (rr_ksplit, rr_combine).
//   latency       the weight loads of 12 blocks x tiles are issued before the first MFMA of a batch (rr_accumulate_nt).
//   LayerNorm     add_layernorm_kernel's formulas (mean, then the biased variance of the differences, rsqrtf(var + eps));
//                 thread (row, part of 32) adds its columns, the 32 parts are added in part order by every thread of the row.
//   relu          fmaxf(v, 0) as bias_act_kernel (NaN -> 0).
// A row's trajectory depends on (Z, d_ff, D, the parameters, its seed) alone: not on n, its index, the grid or the CU count.
//
// seq_spectrum.  out[k] = 1 / (b d) sum_{b,c} | sum_t x[b,t,c] e^{-2 pi i k t / T} |, k = 0..T/2, a direct DFT in fp64.
//   spec_partial  workgroup (16 sequences, 16 columns), 256 threads = 16 columns x 16 frequency groups.  cos / sin(2 pi j / T),
//                 j < T, in fp64 into an LDS table once per workgroup; a sequence's [T][16] tile is staged in LDS; thread
//                 (c, g) walks t ascending for k = g, g + 16, ... with the table index (k t) mod T kept by addition, and adds
//                 the magnitude to its own LDS slot (<= 16 terms).  The 16 columns are added in column order.
//   spec_final    one workgroup per frequency: thread j adds partials j * per .. (j + 1) * per - 1 in order (per <= 4096), a
//                 butterfly across each wave, the four wave sums in wave order, one division by b d.
// No float atomics; grid and orders are functions of (b, T, d) alone: bitwise reproducible across calls and streams.
#include "umlh_common.h"
#include "umlh_launch.h"
#include <algorithm>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int RR_ROWS = 16;               // rows of one workgroup (the N of the MFMA)
constexpr int RR_THREADS = 512;
constexpr int RR_WAVES = RR_THREADS / 64;
constexpr int RR_TG = 4;                  // output tiles a wave accumulates at once
#ifndef RR_PF
#define RR_PF 12
#endif
constexpr int RR_FC_MAX = 512;            // FFN hidden columns per chunk: 512 up to Z = 128, 256 above (rr_fc)
constexpr int RR_REDK = (RR_WAVES - 1) * 256;   // floats of the split products' exchange
constexpr int RR_LN_PARTS = RR_THREADS / RR_ROWS;

struct RolloutArgs {
    const float* p[UMLH_ROLLOUT_MAX_LAYERS][12];
    const float* conv_w;
    const float* pos0;
    const float* w_in;
    const float* b_in;
    const float* w_out;
    const float* b_out;
    const float* x0;
    float* out;
    long long ldx, n, ldb, ldt;
    int Z, dff, D, n_layers, steps;
    float eps;
};

__host__ __device__ __forceinline__ int rr_fc(int Z) { return Z <= 128 ? RR_FC_MAX : RR_FC_MAX / 2; }
__device__ __forceinline__ int rr_pad16(int v) { return (v + 15) & ~15; }
// floats of an activation buffer of width w
__device__ __forceinline__ int rr_buf(int w) { return rr_pad16(w) * RR_ROWS; }
// where element (column c, row r) of an activation lives
__device__ __forceinline__ int rr_at(int c, int r) { return ((c >> 2) * RR_ROWS + r) * 4 + (c & 3); }

// A uniform pointer the optimiser must take as new at this point: without it the address arithmetic of every product of a step
// (per tile, per lane, 64 bits) is hoisted out of the step loop and held in registers across the whole kernel.
__device__ __forceinline__ const float* rr_fresh(const float* p) {
    asm volatile("" : "+s"(p));
    return p;
}

// four adjacent k of one weight row, zeros from k = left on
template <bool VEC>
__device__ __forceinline__ f32x4 rr_load_w(const float* __restrict__ p, const float* __restrict__ safe, int left) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if constexpr (VEC) {                                            // K % 4 == 0: all four or none; the load itself is
        const f32x4 w = *reinterpret_cast<const f32x4*>(left > 0 ? p : safe);      // unconditional (from the row's start
        if (left > 0) v = w;                                         // when there is nothing to take): no branch per load
    } else {
        if (left > 0) v.x = p[0];
        if (left > 1) v.y = p[1];
        if (left > 2) v.z = p[2];
        if (left > 3) v.w = p[3];
    }
    return v;
}

// acc[u] += W[tile_u columns][k_lo + 16 kb0 .. k_lo + min(16 kb1, kn)) . act[16 kb0 ..)   for the wave's NT tiles t0 + 8 u.
// W: row-major [N][ldw]; act: LDS activation whose element 0 is k_lo.  The weight loads of 12 / NT blocks of 16 k go out
// before the first MFMA of the batch: a walk that waits for each block's load is bound by one L2 round trip per block.
template <bool VEC, int NT>
__device__ __forceinline__ void rr_accumulate_nt(const float* __restrict__ W, int ldw, int N, int k_lo, int kn, const float* act,
                                                 int t0, int kb0, int kb1, f32x4 (&acc)[RR_TG]) {
    constexpr int PB = VEC ? RR_PF / NT : (NT > 2 ? 1 : 2);       // unaligned rows: 4-byte loads, a shallower batch
    const int lane = threadIdx.x & 63, m = lane & 15, g = lane >> 4;
    const float* wp[NT];
    const float* row[NT];
#pragma unroll
    for (int u = 0; u < NT; ++u) {
        int col = (t0 + RR_WAVES * u) * 16 + m;
        if (col > N - 1) col = N - 1;                                   // a column past N: its result is dropped
        row[u] = W + (size_t)col * ldw + k_lo;
        wp[u] = row[u] + 4 * g;
    }
    for (int kb = kb0; kb < kb1; kb += PB) {
        f32x4 a[PB][NT];
#pragma unroll
        for (int j = 0; j < PB; ++j) {
            const int left = kb + j < kb1 ? kn - ((kb + j) * 16 + 4 * g) : 0;
#pragma unroll
            for (int u = 0; u < NT; ++u) a[j][u] = rr_load_w<VEC>(wp[u] + (kb + j) * 16, row[u], left);
        }
#pragma unroll
        for (int j = 0; j < PB; ++j) {
            if (kb + j < kb1) {                                          // wave-uniform
                const f32x4 b = *reinterpret_cast<const f32x4*>(act + (((kb + j) * 4 + g) * RR_ROWS + m) * 4);
#pragma unroll
                for (int u = 0; u < NT; ++u) {
                    acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j][u].x, b.x, acc[u], 0, 0, 0);
                    acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j][u].y, b.y, acc[u], 0, 0, 0);
                    acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j][u].z, b.z, acc[u], 0, 0, 0);
                    acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j][u].w, b.w, acc[u], 0, 0, 0);
                }
            }
        }
    }
    // the accumulators are read right behind the last MFMA of a chain: keep the result latency of v_mfma_f32_16x16x4_f32
    // covered whatever the compiler schedules next (see the note in umlh_kernels_micro.hip)
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 7" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// the wave's live tiles t0 + 8 u < nt (at most RR_TG), blocks kb0 .. kb1 - 1 of the reduction
template <bool VEC>
__device__ __forceinline__ void rr_accumulate(const float* __restrict__ W, int ldw, int N, int k_lo, int kn, const float* act,
                                              int t0, int nt, int kb0, int kb1, f32x4 (&acc)[RR_TG]) {
    const int live = (nt - t0 + RR_WAVES - 1) / RR_WAVES;               // wave-uniform
    if (live >= 4) rr_accumulate_nt<VEC, 4>(W, ldw, N, k_lo, kn, act, t0, kb0, kb1, acc);
    else if (live == 3) rr_accumulate_nt<VEC, 3>(W, ldw, N, k_lo, kn, act, t0, kb0, kb1, acc);
    else if (live == 2) rr_accumulate_nt<VEC, 2>(W, ldw, N, k_lo, kn, act, t0, kb0, kb1, acc);
    else if (live == 1) rr_accumulate_nt<VEC, 1>(W, ldw, N, k_lo, kn, act, t0, kb0, kb1, acc);
}

// Narrow outputs (fewer tiles than waves) split the reduction across waves: ks = min(8 / nt, nkb / 4) parts of ceil(nkb / ks)
// blocks, part p on wave p nt + tile, the parts' sums added in part order by part 0 (rr_combine).  A function of (N, K) alone.
__device__ __forceinline__ int rr_ksplit(int nt, int nkb) {
    if (nt >= RR_WAVES) return 1;
    int ks = RR_WAVES / nt;
    if (ks > nkb / 4) ks = nkb / 4;
    return ks < 1 ? 1 : ks;
}

struct RrPart {
    int t0, part, kb0, kb1;
    bool active;
};

// the wave's share of a split product with nkb blocks (ks > 1)
__device__ __forceinline__ RrPart rr_part(int nt, int nkb, int ks) {
    const int wave = threadIdx.x >> 6, per = (nkb + ks - 1) / ks;
    RrPart p;
    p.active = wave < nt * ks;
    p.t0 = wave % nt;
    p.part = wave / nt;
    p.kb0 = p.part * per;
    p.kb1 = p.kb0 + per < nkb ? p.kb0 + per : nkb;
    return p;
}

// part 0's acc[0] += the other parts' acc[0] in part order; redk: (ks - 1) * nt * 256 floats.  One workgroup barrier inside.
__device__ __forceinline__ void rr_combine(const RrPart& p, int nt, int ks, float* redk, f32x4 (&acc)[RR_TG]) {
    const int lane = threadIdx.x & 63;
    if (p.active && p.part > 0) *reinterpret_cast<f32x4*>(redk + (((p.part - 1) * nt + p.t0) * 64 + lane) * 4) = acc[0];
    __syncthreads();
    if (p.active && p.part == 0)
        for (int q = 1; q < ks; ++q) acc[0] += *reinterpret_cast<const f32x4*>(redk + (((q - 1) * nt + p.t0) * 64 + lane) * 4);
}

// dst tile <- epi(column, acc element) for the wave's live tiles; columns >= N are written as zeros.
// epi(c, v, r) -> float: c the output column, v the sum, r the row of the workgroup.
template <class Epi>
__device__ __forceinline__ void rr_store(float* dst, int N, int t0, int nt, const f32x4 (&acc)[RR_TG], Epi epi) {
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
#pragma unroll
    for (int u = 0; u < RR_TG; ++u) {
        const int tile = t0 + RR_WAVES * u;
        if (tile < nt) {
            const int c = tile * 16 + 4 * g;
            f32x4 v;
            v.x = c + 0 < N ? epi(c + 0, acc[u].x, r) : 0.f;
            v.y = c + 1 < N ? epi(c + 1, acc[u].y, r) : 0.f;
            v.z = c + 2 < N ? epi(c + 2, acc[u].z, r) : 0.f;
            v.w = c + 3 < N ? epi(c + 3, acc[u].w, r) : 0.f;
            *reinterpret_cast<f32x4*>(dst + ((tile * 4 + g) * RR_ROWS + r) * 4) = v;
        }
    }
}

// dst[N][16] = epi(W[N][K] . act[K][16]); all waves, any N.  Ends with a workgroup barrier.
template <class Epi>
__device__ __forceinline__ void rr_linear(const float* __restrict__ W, int N, int K, const float* act, float* dst, float* redk, Epi epi) {
    const int wave = threadIdx.x >> 6, nt = (N + 15) >> 4, nkb = (K + 15) >> 4;
    const bool vec = (K & 3) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0;
    const int ks = rr_ksplit(nt, nkb);
    f32x4 acc[RR_TG];
    if (ks > 1) {
        const RrPart p = rr_part(nt, nkb, ks);
#pragma unroll
        for (int u = 0; u < RR_TG; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (p.active) {
            if (vec) rr_accumulate_nt<true, 1>(W, K, N, 0, K, act, p.t0, p.kb0, p.kb1, acc);
            else rr_accumulate_nt<false, 1>(W, K, N, 0, K, act, p.t0, p.kb0, p.kb1, acc);
        }
        rr_combine(p, nt, ks, redk, acc);
        if (p.active && p.part == 0) rr_store(dst, N, p.t0, nt, acc, epi);
    } else {
        for (int t0 = wave; t0 < nt; t0 += RR_WAVES * RR_TG) {
#pragma unroll
            for (int u = 0; u < RR_TG; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (vec) rr_accumulate<true>(W, K, N, 0, K, act, t0, nt, 0, nkb, acc);
            else rr_accumulate<false>(W, K, N, 0, K, act, t0, nt, 0, nkb, acc);
            rr_store(dst, N, t0, nt, acc, epi);
        }
    }
    __syncthreads();
}

// h <- LayerNorm(s) * gamma + beta over Z columns, pad columns of h zeroed.  red: 2 * RR_THREADS floats.  Ends with a barrier.
__device__ __forceinline__ void rr_layernorm(const float* s, float* h, const float* __restrict__ gamma,
                                             const float* __restrict__ beta, int Z, float eps, float* red) {
    const int tid = threadIdx.x, r = tid & 15, part = tid >> 4, nq = rr_pad16(Z) >> 2;
    float sum = 0.f;
    for (int q = part; q < nq; q += RR_LN_PARTS) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(s + (q * RR_ROWS + r) * 4);
        const int c = 4 * q;
        if (c + 0 < Z) sum += v.x;
        if (c + 1 < Z) sum += v.y;
        if (c + 2 < Z) sum += v.z;
        if (c + 3 < Z) sum += v.w;
    }
    red[part * RR_ROWS + r] = sum;
    __syncthreads();
    float tot = 0.f;
    for (int p = 0; p < RR_LN_PARTS; ++p) tot += red[p * RR_ROWS + r];
    const float mean = tot / (float)Z;
    float var = 0.f;
    for (int q = part; q < nq; q += RR_LN_PARTS) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(s + (q * RR_ROWS + r) * 4);
        const int c = 4 * q;
        float d;
        if (c + 0 < Z) { d = v.x - mean; var += d * d; }
        if (c + 1 < Z) { d = v.y - mean; var += d * d; }
        if (c + 2 < Z) { d = v.z - mean; var += d * d; }
        if (c + 3 < Z) { d = v.w - mean; var += d * d; }
    }
    float* red2 = red + RR_THREADS;
    red2[part * RR_ROWS + r] = var;
    __syncthreads();
    float vt = 0.f;
    for (int p = 0; p < RR_LN_PARTS; ++p) vt += red2[p * RR_ROWS + r];
    const float rstd = rsqrtf(vt / (float)Z + eps);
    for (int q = part; q < nq; q += RR_LN_PARTS) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(s + (q * RR_ROWS + r) * 4);
        const int c = 4 * q;
        f32x4 y;
        y.x = c + 0 < Z ? (v.x - mean) * rstd * gamma[c + 0] + beta[c + 0] : 0.f;
        y.y = c + 1 < Z ? (v.y - mean) * rstd * gamma[c + 1] + beta[c + 1] : 0.f;
        y.z = c + 2 < Z ? (v.z - mean) * rstd * gamma[c + 2] + beta[c + 2] : 0.f;
        y.w = c + 3 < Z ? (v.w - mean) * rstd * gamma[c + 3] + beta[c + 3] : 0.f;
        *reinterpret_cast<f32x4*>(h + (q * RR_ROWS + r) * 4) = y;
    }
    __syncthreads();
}

// out[row0 + r, s, :] <- cur (rows < n only)
__device__ __forceinline__ void rr_emit(const RolloutArgs& a, const float* cur, long long row0, int s) {
    const int total = RR_ROWS * a.D;
    for (int i = threadIdx.x; i < total; i += RR_THREADS) {
        const int r = i / a.D, c = i - r * a.D;
        if (row0 + r < a.n) a.out[(row0 + r) * a.ldb + (long long)s * a.ldt + c] = cur[rr_at(c, r)];
    }
}

__global__ __launch_bounds__(RR_THREADS) void rollout_rows(const RolloutArgs a) {
    extern __shared__ __attribute__((aligned(16))) float rr_lds[];
    const int Z = a.Z, D = a.D, dff = a.dff;
    // bufA | bufB | U = max(cur, s + hid) | red:  cur is dead while a step's layers run, s and hid while it is produced and read
    float* bufA = rr_lds;
    float* bufB = bufA + rr_buf(Z);
    float* U = bufB + rr_buf(Z);
    float* cur = U;
    float* sres = U;
    float* hid = U + rr_buf(Z);
    const int FC = rr_fc(Z);
    const int ulen = rr_buf(D) > rr_buf(Z) + FC * RR_ROWS ? rr_buf(D) : rr_buf(Z) + FC * RR_ROWS;
    float* red = U + ulen;
    float* redk = red + 2 * RR_THREADS;
    const long long row0 = (long long)blockIdx.x * RR_ROWS;
    const int tid = threadIdx.x, wave = tid >> 6;

    for (int i = tid; i < rr_buf(D); i += RR_THREADS) {                  // the seed, zeros past D and past n
        const int q = i >> 6, r = (i >> 2) & 15, c = 4 * q + (i & 3);
        cur[i] = (c < D && row0 + r < a.n) ? a.x0[(row0 + r) * a.ldx + c] : 0.f;
    }
    __syncthreads();
    rr_emit(a, cur, row0, 0);

    for (int s = 1; s <= a.steps; ++s) {
        float* h = bufA;
        float* other = bufB;
        {
            const float* b_in = a.b_in;
            const float* pos = a.conv_w ? nullptr : a.pos0;
            rr_linear(rr_fresh(a.w_in), Z, D, cur, h, redk, [=](int c, float v, int) { return pos ? (v + b_in[c]) + pos[c] : v + b_in[c]; });
        }
        if (a.conv_w) {
            const float* pos = a.pos0;
            rr_linear(rr_fresh(a.conv_w), Z, Z, h, other, redk, [=](int c, float v, int) { return pos ? v + pos[c] : v; });
            float* t = h; h = other; other = t;
        }
        for (int l = 0; l < a.n_layers; ++l) {
            const float* const* P = a.p[l];
            {
                const float* bv = P[1] + 2 * Z;
                rr_linear(rr_fresh(P[0]) + (size_t)2 * Z * Z, Z, Z, h, other, redk, [=](int c, float v, int) { return v + bv[c]; });
            }
            {
                const float* bo = P[3];
                const float* hh = h;
                rr_linear(rr_fresh(P[2]), Z, Z, other, sres, redk, [=](int c, float v, int r) { return hh[rr_at(c, r)] + (v + bo[c]); });
            }
            rr_layernorm(sres, h, P[8], P[9], Z, a.eps, red);
            // FFN: hidden columns in chunks of FC, the second product's accumulators carried across the chunks (and, where it is
            // split across waves, combined once at the end: the split is that of a full chunk, the same for every chunk)
            const int ntz = (Z + 15) >> 4;
            const int ks2 = rr_ksplit(ntz, ((dff < FC ? dff : FC) + 15) >> 4);
            f32x4 acc[RR_TG];
#pragma unroll
            for (int u = 0; u < RR_TG; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            const float* W2_layer = P[6];
            const bool vec2 = (dff & 3) == 0 && (reinterpret_cast<uintptr_t>(W2_layer) & 15) == 0;
            RrPart p2 = {wave, 0, 0, 0, wave < ntz};
            for (int f0 = 0; f0 < dff; f0 += FC) {
                const int fn = dff - f0 < FC ? dff - f0 : FC;
                const float* b1 = P[5] + f0;
                rr_linear(rr_fresh(P[4]) + (size_t)f0 * Z, fn, Z, h, hid, redk, [=](int c, float v, int) { return fmaxf(v + b1[c], 0.f); });
                const int nkb = (fn + 15) >> 4;
                const float* W2 = rr_fresh(W2_layer);
                if (ks2 > 1) {
                    p2 = rr_part(ntz, nkb, ks2);
                    if (p2.active) {
                        if (vec2) rr_accumulate_nt<true, 1>(W2, dff, Z, f0, fn, hid, p2.t0, p2.kb0, p2.kb1, acc);
                        else rr_accumulate_nt<false, 1>(W2, dff, Z, f0, fn, hid, p2.t0, p2.kb0, p2.kb1, acc);
                    }
                } else if (wave < ntz) {
                    if (vec2) rr_accumulate<true>(W2, dff, Z, f0, fn, hid, wave, ntz, 0, nkb, acc);
                    else rr_accumulate<false>(W2, dff, Z, f0, fn, hid, wave, ntz, 0, nkb, acc);
                }
                __syncthreads();                                          // hid is rewritten by the next chunk
            }
            {
                const float* b2 = P[7];
                const float* hh = h;
                if (ks2 > 1) rr_combine(p2, ntz, ks2, redk, acc);
                if (p2.active && p2.part == 0)
                    rr_store(sres, Z, p2.t0, ntz, acc, [=](int c, float v, int r) { return hh[rr_at(c, r)] + (v + b2[c]); });
                __syncthreads();
            }
            rr_layernorm(sres, h, P[10], P[11], Z, a.eps, red);
        }
        {
            const float* bo = a.b_out;
            rr_linear(rr_fresh(a.w_out), D, Z, h, cur, redk, [=](int c, float v, int) { return v + bo[c]; });
        }
        rr_emit(a, cur, row0, s);
    }
}

inline size_t rr_lds_bytes(int Z, int dff, int D) {
    auto buf = [](int w) { return (size_t)((w + 15) & ~15) * RR_ROWS; };
    const size_t u = std::max(buf(D), buf(Z) + (size_t)rr_fc(Z) * RR_ROWS);
    (void)dff;
    return (2 * buf(Z) + u + 2 * RR_THREADS + RR_REDK) * sizeof(float);
}

// ---- seq_spectrum ----
constexpr int SP_SEQS = 16;               // sequences per workgroup
constexpr int SP_COLS = 16;               // columns per workgroup
constexpr int SP_THREADS = 256;
constexpr int SP_FINAL_THREADS = 256;
constexpr int SP_FINAL_CHAIN = 4096;
constexpr long long SP_MAX_PARTIALS = (long long)SP_FINAL_THREADS * SP_FINAL_CHAIN;

__global__ __launch_bounds__(SP_THREADS) void spec_partial(const float* __restrict__ x, long long ldb, long long ldt, int B, int T, int d,
                                                           int col_chunks, double* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sp_lds[];
    const int K = T / 2 + 1;
    double* tw_c = reinterpret_cast<double*>(sp_lds);                    // [T]
    double* tw_s = tw_c + T;                                             // [T]
    double* mag = tw_s + T;                                              // [K][SP_COLS]
    float* tile = reinterpret_cast<float*>(mag + (size_t)K * SP_COLS);   // [T][SP_COLS]
    const int tid = threadIdx.x, c = tid & (SP_COLS - 1), g = tid / SP_COLS;
    const int bc = blockIdx.x / col_chunks, cc = blockIdx.x - bc * col_chunks;
    for (int j = tid; j < T; j += SP_THREADS) {
        double sn, cs;
        sincospi(2.0 * (double)j / (double)T, &sn, &cs);
        tw_c[j] = cs;
        tw_s[j] = sn;
    }
    for (int i = tid; i < K * SP_COLS; i += SP_THREADS) mag[i] = 0.0;
    const int b_end = (bc + 1) * SP_SEQS < B ? (bc + 1) * SP_SEQS : B;
    for (int b = bc * SP_SEQS; b < b_end; ++b) {
        __syncthreads();                                                 // the table (first pass), the tile's last readers
        for (int i = tid; i < T * SP_COLS; i += SP_THREADS) {
            const int t = i / SP_COLS, cj = cc * SP_COLS + (i & (SP_COLS - 1));
            tile[i] = cj < d ? x[(long long)b * ldb + (long long)t * ldt + cj] : 0.f;
        }
        __syncthreads();
        for (int k = g; k < K; k += SP_THREADS / SP_COLS) {
            double re = 0.0, im = 0.0;
            int idx = 0;
            for (int t = 0; t < T; ++t) {
                const double v = (double)tile[t * SP_COLS + c];
                re += v * tw_c[idx];
                im -= v * tw_s[idx];
                idx += k;
                if (idx >= T) idx -= T;
            }
            mag[k * SP_COLS + c] += sqrt(re * re + im * im);             // this thread's own slot
        }
    }
    __syncthreads();
    for (int k = tid; k < K; k += SP_THREADS) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < SP_COLS; ++j) s += mag[k * SP_COLS + j];
        partial[(long long)blockIdx.x * K + k] = s;
    }
}

__global__ __launch_bounds__(SP_FINAL_THREADS) void spec_final(const double* __restrict__ partial, long long n_partials, int K,
                                                               double count, double* __restrict__ out) {
    __shared__ double wsum[SP_FINAL_THREADS / 64];
    const int tid = threadIdx.x, k = blockIdx.x;
    const long long per = (n_partials + SP_FINAL_THREADS - 1) / SP_FINAL_THREADS;
    long long hi = (tid + 1) * per;
    if (hi > n_partials) hi = n_partials;
    double s = 0.0;
    for (long long i = tid * per; i < hi; ++i) s += partial[i * K + k];
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m, 64);
    if ((tid & 63) == 0) wsum[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) out[k] = (((wsum[0] + wsum[1]) + wsum[2]) + wsum[3]) / count;
}

inline size_t sp_lds_bytes(int T) {
    const size_t K = (size_t)T / 2 + 1;
    return 2 * (size_t)T * sizeof(double) + K * SP_COLS * sizeof(double) + (size_t)T * SP_COLS * sizeof(float);
}

}  // namespace

// LDS bytes of one rollout workgroup at this shape (the API compares it with UMLH_ROLLOUT_MAX_LDS)
extern "C" unsigned long long umlh_rollout_lds_bytes(int Z, int dff, int D) { return rr_lds_bytes(Z, dff, D); }

extern "C" int umlh_rollout_launch(const umlh_rollout_cfg_t* cfg, const float* const* P, const float* conv_w, const float* pos0,
                                   const float* w_in, const float* b_in, const float* w_out, const float* b_out, const float* x0,
                                   long long ldx, long long n, float* out, long long ldb, long long ldt, hipStream_t st) {
    if (int e = raise_lds_limit<&rollout_rows>(UMLH_ROLLOUT_MAX_LDS)) return e;
    RolloutArgs a;
    for (int l = 0; l < UMLH_ROLLOUT_MAX_LAYERS; ++l)
        for (int j = 0; j < 12; ++j) a.p[l][j] = l < cfg->n_layers ? P[12 * l + j] : nullptr;
    a.conv_w = conv_w; a.pos0 = pos0; a.w_in = w_in; a.b_in = b_in; a.w_out = w_out; a.b_out = b_out;
    a.x0 = x0; a.out = out; a.ldx = ldx; a.n = n; a.ldb = ldb; a.ldt = ldt;
    a.Z = cfg->Z; a.dff = cfg->d_ff; a.D = cfg->D; a.n_layers = cfg->n_layers; a.steps = cfg->steps; a.eps = cfg->eps;
    const unsigned grid = (unsigned)((n + RR_ROWS - 1) / RR_ROWS);
    hipLaunchKernelGGL(rollout_rows, dim3(grid), dim3(RR_THREADS), rr_lds_bytes(a.Z, a.dff, a.D), st, a);
    return (int)hipGetLastError();
}

// partial vectors of one spectrum call: ceil(b / 16) * ceil(d / 16); -1 when the final's chains would pass 4096 terms
extern "C" long long umlh_spectrum_partials(int B, int T, int d) {
    (void)T;
    const long long p = (((long long)B + SP_SEQS - 1) / SP_SEQS) * (((long long)d + SP_COLS - 1) / SP_COLS);
    return p > SP_MAX_PARTIALS ? -1 : p;
}

extern "C" unsigned long long umlh_spectrum_bytes(int B, int T, int d) {
    const long long p = umlh_spectrum_partials(B, T, d);
    return (unsigned long long)align_up((p > 0 ? p : 1) * (T / 2 + 1) * 8);
}

extern "C" int umlh_spectrum_launch(const float* x, long long ldb, long long ldt, int B, int T, int d, double* out, void* scratch,
                                    hipStream_t st) {
    if (int e = raise_lds_limit<&spec_partial>((int)sp_lds_bytes(UMLH_SPECTRUM_MAX_T))) return e;
    double* partial = at<double>(scratch, 0);
    const long long p = umlh_spectrum_partials(B, T, d);
    const int col_chunks = (d + SP_COLS - 1) / SP_COLS, K = T / 2 + 1;
    hipLaunchKernelGGL(spec_partial, dim3((unsigned)p), dim3(SP_THREADS), sp_lds_bytes(T), st, x, ldb, ldt, B, T, d, col_chunks, partial);
    hipLaunchKernelGGL(spec_final, dim3((unsigned)K), dim3(SP_FINAL_THREADS), 0, st, (const double*)partial, p, K,
                       (double)B * (double)d, out);
    return (int)hipGetLastError();
}
