// Outlier clamp and feature preparation of the alignment metrics (vision_language/metrics.py:327-341 remove_outliers,
// :258-269 compute_knn_accuracy).  Kernels:
//   row_select     per row, the order statistics s[lo], s[hi] of the ascending |x| and the interpolated quantile
//   quant_partial  fixed-order double sums of 4096 row quantiles each
//   quant_final    fixed-order sum of those -> mean64, q_val
//   kth_pass<P>    one radix pass of the global k-th of |x|; the workgroup that takes the last ticket picks the digit
//   clamp_flat     out = clamp(x, -q_val, q_val)
//   clamp_norm     the same and the division by max(|row|_2, 1e-12) in one launch
//   acc_count      rows i of an int32 list that contain i, integer block sums
//   acc_final      fixed-order sum of the block counts -> mean as double
//
// Selection is an MSB-first radix select on key = bits(x) & 0x7fffffff, whose unsigned order is the order of |x| with the NaN
// patterns above Inf.  Four passes take the digits key[30:23], [22:15], [14:7], [6:0]; a pass counts the keys that agree with
// the digits chosen so far into 256 integer counters (LDS atomics), and one wave scans the counters for the digit that holds
// the wanted rank.  After the last pass the key s[lo] is known with the number of keys equal to it and the rank inside them:
// s[lo + 1] is the same key when that rank is not the last of them, else the smallest key above it (one more sweep, an LDS
// integer atomicMin).  Nothing here sums floats with atomics and no workgroup waits for another.
#include "umlh_common.h"
#include "umlh_launch.h"

namespace {

constexpr int WAVE_COLS = UMLH_ROW_QUANTILE_WAVE_COLS;     // up to here a wave per row, four rows per workgroup
constexpr int LDS_COLS = UMLH_ROW_QUANTILE_LDS_COLS;       // up to here the row is read once and kept in LDS (60 KiB: two workgroups per CU)
constexpr unsigned ABS_MASK = 0x7fffffffu, INF_KEY = 0x7f800000u;
constexpr int QUANT_CHUNK = 4096;                          // row quantiles per partial sum

__device__ __forceinline__ unsigned abs_key(float v) { return __builtin_bit_cast(unsigned, v) & ABS_MASK; }
// pass p: a key takes part when its bits above the digit equal the prefix's; the digit is (key >> lo_shift) & mask
__device__ __forceinline__ int hi_shift(int p) { return 31 - 8 * p; }
__device__ __forceinline__ int lo_shift(int p) { return p == 3 ? 0 : 23 - 8 * p; }
__device__ __forceinline__ unsigned digit_mask(int p) { return p == 3 ? 127u : 255u; }

// s[lo] + (s[hi] - s[lo]) * frac in double, every operation rounded on its own (no fused multiply-add: the product is rounded
// before the sum, as the float64 statement of the contract does), then rounded once to fp32
__device__ __forceinline__ float interpolate(float a, float b, double frac) {
#pragma clang fp contract(off)
    const double diff = (double)b - (double)a;
    const double prod = diff * frac;
    return (float)((double)a + prod);
}

// One wave: the digit whose counters cover `rank` (lane l scans counters 4l .. 4l+3; exactly one lane finds it, because the
// counters sum to more than rank).  found -> {digit, counters below it, counter of it}.
template <class T>
__device__ __forceinline__ bool scan_digit(const T c[4], T rank, int lane, int& digit, T& below, T& count) {
    const T s = c[0] + c[1] + c[2] + c[3];
    T incl = s;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    T excl = incl - s;
    if (!(excl <= rank && rank < incl)) return false;
    int j = 0;
    while (rank >= excl + c[j]) { excl += c[j]; ++j; }      // j <= 3: rank < incl
    digit = 4 * lane + j; below = excl; count = c[j];
    return true;
}

// ROWS rows per workgroup, G = THREADS / ROWS threads (whole waves) per row.  COLS > 0: the row's keys are read once into LDS;
// COLS == 0: every pass streams the row again.  Every thread reaches every barrier, whatever its row holds.
template <int THREADS, int ROWS, int COLS>
__global__ __launch_bounds__(THREADS) void row_select(const float* __restrict__ x, long long n, int d, long long ld, int lo, int hi,
                                                      double frac, float* __restrict__ lo_val, float* __restrict__ hi_val,
                                                      float* __restrict__ quant) {
    constexpr int G = THREADS / ROWS;
    static_assert(G % 64 == 0, "whole waves per row");
    __shared__ unsigned keys[ROWS][COLS > 0 ? COLS : 1];
    __shared__ unsigned hist[ROWS][256];
    __shared__ unsigned st[ROWS][4];                       // prefix, rank, count, unused
    __shared__ unsigned aux[ROWS][2];                      // NaN seen, smallest key above s[lo]
    const int g = threadIdx.x / G, gid = threadIdx.x % G;
    const long long row_blocks = (n + ROWS - 1) / ROWS;
    for (long long rb = blockIdx.x; rb < row_blocks; rb += gridDim.x) {
        const long long row = rb * ROWS + g;
        const bool active = row < n;
        const float* xr = x + (active ? row : 0) * ld;
        __syncthreads();                                   // the previous row block is done with the LDS
        if (gid == 0) { aux[g][0] = 0u; aux[g][1] = 0xffffffffu; }
        bool nan = false;
        if (COLS > 0) {
            for (int j = gid; j < d; j += G) {
                const unsigned k = abs_key(xr[j]);
                keys[g][j] = k;
                nan |= k > INF_KEY;
            }
        }
        auto key_at = [&](int j) { return COLS > 0 ? keys[g][j] : abs_key(xr[j]); };
        unsigned prefix = 0u, rank = (unsigned)lo, count = 0u;
        for (int p = 0; p < 4; ++p) {
            for (int b = gid; b < 256; b += G) hist[g][b] = 0u;
            __syncthreads();
            const int hs = hi_shift(p), ls = lo_shift(p);
            const unsigned mask = digit_mask(p), want = prefix >> hs;
            for (int j = gid; j < d; j += G) {
                const unsigned k = key_at(j);
                if (COLS == 0 && p == 0) nan |= k > INF_KEY;
                if ((k >> hs) == want) atomicAdd(&hist[g][(k >> ls) & mask], 1u);
            }
            if (p == 0 && nan) atomicOr(&aux[g][0], 1u);
            __syncthreads();
            if (gid < 64) {
                const unsigned c[4] = {hist[g][4 * gid], hist[g][4 * gid + 1], hist[g][4 * gid + 2], hist[g][4 * gid + 3]};
                int digit;
                unsigned below, cnt;
                if (scan_digit(c, rank, gid, digit, below, cnt)) {
                    st[g][0] = prefix | ((unsigned)digit << ls);
                    st[g][1] = rank - below;
                    st[g][2] = cnt;
                }
            }
            __syncthreads();
            prefix = st[g][0]; rank = st[g][1]; count = st[g][2];
        }
        // prefix = s[lo]; `count` keys equal it and s[lo] is number `rank` of them
        const bool need_next = hi != lo && rank + 1u >= count;
        if (need_next) {
            unsigned m = 0xffffffffu;
            for (int j = gid; j < d; j += G) {
                const unsigned k = key_at(j);
                if (k > prefix && k < m) m = k;
            }
            if (m != 0xffffffffu) atomicMin(&aux[g][1], m);
        }
        __syncthreads();
        if (gid == 0 && active) {
            const unsigned khi = need_next ? aux[g][1] : prefix;
            const float a = __builtin_bit_cast(float, prefix), b = __builtin_bit_cast(float, khi);
            if (lo_val) lo_val[row] = a;
            if (hi_val) hi_val[row] = b;
            quant[row] = aux[g][0] ? __builtin_nanf("") : interpolate(a, b, frac);
        }
    }
}

// partial[b] = sum of quant[b * 4096 ..) in a fixed order: thread t adds rows t, t + 256, ... then the halving tree
__global__ __launch_bounds__(256) void quant_partial(const float* __restrict__ quant, long long n, double* __restrict__ partial) {
    __shared__ double red[256];
    const long long base = (long long)blockIdx.x * QUANT_CHUNK;
    double s = 0.0;
    for (int j = threadIdx.x; j < QUANT_CHUNK && base + j < n; j += 256) s += (double)quant[base + j];
    s = block_reduce<256>(s, red, OpSum());
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void quant_final(const double* __restrict__ partial, long long nparts, long long n,
                                                   double* __restrict__ mean64, float* __restrict__ q_val) {
    __shared__ double red[256];
    double s = 0.0;
    for (long long j = threadIdx.x; j < nparts; j += 256) s += partial[j];
    s = block_reduce<256>(s, red, OpSum());
    if (threadIdx.x == 0) {
        const double m = s / (double)n;
        if (mean64) mean64[0] = m;
        q_val[0] = (float)m;
    }
}

// ---- global k-th: the same four passes across workgroups, one launch each ----
struct KthState { unsigned long long prefix, consumed; unsigned ticket[4]; };

constexpr int KTH_THREADS = 1024;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// nvec > 0: the matrix is dense (ld == d) on a 16-byte base and is read as nvec 16-byte words, the last total - 4 nvec elements by
// workgroup 0; else element e is x[(e / d) * ld + e % d], four independent loads in flight per thread.  Few, large workgroups:
// every one of them adds up to 256 counters into the same 2 KiB of global memory.  Each wave counts into its own 256 LDS
// counters (the top digit of real features is the exponent: a handful of hot counters) and the workgroup sums them at the end.
template <int PASS>
__global__ __launch_bounds__(KTH_THREADS) void kth_pass(const float* __restrict__ x, long long total, long long d, long long ld,
                                                        long long nvec, unsigned long long k, unsigned long long* __restrict__ ghist,
                                                        KthState* __restrict__ st, float* __restrict__ out) {
    __shared__ unsigned lh[KTH_THREADS / 64][256];           // counters of each wave's own: no two waves add to one LDS word
    __shared__ int last;
    const int tid = threadIdx.x, wave = tid >> 6;
    const unsigned prefix = (unsigned)st->prefix;          // written by the previous pass's launch
    const int hs = hi_shift(PASS), ls = lo_shift(PASS);
    const unsigned mask = digit_mask(PASS), want = prefix >> hs;
    for (int b = tid & 63; b < 256; b += 64) lh[wave][b] = 0u;
    __syncthreads();
    auto count = [&](unsigned bits) {
        const unsigned key = bits & ABS_MASK;
        if ((key >> hs) == want) atomicAdd(&lh[wave][(key >> ls) & mask], 1u);
    };
    const long long step = (long long)gridDim.x * KTH_THREADS, first = (long long)blockIdx.x * KTH_THREADS + tid;
    if (nvec > 0) {
        const u32x4* xv = reinterpret_cast<const u32x4*>(x);
        for (long long i = first; i < nvec; i += 2 * step) {
            const u32x4 a = xv[i];
            const bool two = i + step < nvec;
            const u32x4 b = two ? xv[i + step] : a;
            count(a[0]); count(a[1]); count(a[2]); count(a[3]);
            if (two) { count(b[0]); count(b[1]); count(b[2]); count(b[3]); }
        }
        if (blockIdx.x == 0)
            for (long long e = nvec * 4 + tid; e < total; e += KTH_THREADS) count(__builtin_bit_cast(unsigned, x[e]));
    } else {
        for (long long e = first; e < total; e += 4 * step) {
            bool on[4];
            unsigned v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long long eu = e + u * step;
                on[u] = eu < total;
                v[u] = on[u] ? __builtin_bit_cast(unsigned, x[ld == d ? eu : (eu / d) * ld + eu % d]) : 0u;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (on[u]) count(v[u]);
        }
    }
    __syncthreads();
    unsigned long long* gh = ghist + PASS * 256;
    if (tid < 256) {
        unsigned long long c = 0;
#pragma unroll
        for (int w = 0; w < KTH_THREADS / 64; ++w) c += lh[w][tid];
        if (c) atomicAdd(&gh[tid], c);
    }
    // One release per workgroup, not one fence per wave (an agent-scope fence writes back and invalidates the XCD's L2: with
    // every wave fencing, a pass took 60 ns per wave whatever it read).  Every wave's counter adds have completed before the
    // barrier; thread 0's release-acquire ticket orders them before the last workgroup's reads.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0)
        last = __hip_atomic_fetch_add(&st->ticket[PASS], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
    __syncthreads();
    if (!last || tid >= 64) return;
    unsigned long long c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = __hip_atomic_load(&gh[4 * tid + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long consumed = st->consumed;
    int digit;
    unsigned long long below, cnt;
    if (scan_digit(c, k - consumed, tid, digit, below, cnt)) {
        const unsigned np = prefix | ((unsigned)digit << ls);
        st->prefix = np;
        st->consumed = consumed + below;
        if (PASS == 3) out[0] = __builtin_bit_cast(float, np);
    }
}

// torch.clamp(x, -q, q) with tensor bounds: a NaN x stays, a NaN bound makes everything NaN, else min(max(x, -q), q) with
// std::max / std::min's choice among equals (-0.0 stays -0.0)
__device__ __forceinline__ float clamp1(float v, float q) {
    if (v != v) return v;
    if (q != q) return __builtin_nanf("");
    const float lo = -q;
    v = v < lo ? lo : v;
    return q < v ? q : v;
}

// rows of d columns in chunks of 1024; a dense pair (ldx == d == ldo) comes as one row of n * d
__global__ __launch_bounds__(256) void clamp_flat(const float* x, long long n, long long d, long long ldx, const float* __restrict__ qv,
                                                  float* out, long long ldo, long long nvec) {
    const float q = qv[0];
    const int tid = threadIdx.x;
    if (nvec > 0) {                                        // dense, both bases on 16 bytes: 16-byte accesses, the tail below
        const f32x4v* xv = reinterpret_cast<const f32x4v*>(x);
        f32x4v* ov = reinterpret_cast<f32x4v*>(out);
        for (long long i = (long long)blockIdx.x * 256 + tid; i < nvec; i += (long long)gridDim.x * 256) {
            f32x4v v = xv[i];
            v[0] = clamp1(v[0], q); v[1] = clamp1(v[1], q); v[2] = clamp1(v[2], q); v[3] = clamp1(v[3], q);
            ov[i] = v;
        }
        if (blockIdx.x == 0)
            for (long long j = nvec * 4 + tid; j < d; j += 256) out[j] = clamp1(x[j], q);
        return;
    }
    const long long chunks = (d + 1023) / 1024, items = n * chunks;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const long long row = it / chunks, c0 = (it % chunks) * 1024;
        const float* xr = x + row * ldx;
        float* orow = out + row * ldo;
        for (long long j = c0 + tid; j < d && j < c0 + 1024; j += 256) orow[j] = clamp1(xr[j], q);
    }
}

// clamp and F.normalize(dim=-1) of ROWS rows per workgroup.  COLS > 0: the clamped row waits in LDS between the two sweeps;
// COLS == 0: x is read twice (in place that is safe: a thread writes only what it has read).  |row|^2 in double in a fixed
// order: thread gid adds columns gid, gid + G, ..., a wave's lanes in the xor butterfly, the row's waves in ascending order.
template <int THREADS, int ROWS, int COLS>
__global__ __launch_bounds__(THREADS) void clamp_norm(const float* x, long long n, int d, long long ldx, const float* __restrict__ qv,
                                                      float* out, long long ldo) {
    constexpr int G = THREADS / ROWS, WAVES = G / 64;
    static_assert(G % 64 == 0, "whole waves per row");
    __shared__ float held[ROWS][COLS > 0 ? COLS : 1];
    __shared__ double red[ROWS][WAVES];
    const float q = qv[0];
    const int g = threadIdx.x / G, gid = threadIdx.x % G;
    const long long row_blocks = (n + ROWS - 1) / ROWS;
    for (long long rb = blockIdx.x; rb < row_blocks; rb += gridDim.x) {
        const long long row = rb * ROWS + g;
        const bool active = row < n;
        const float* xr = x + (active ? row : 0) * ldx;
        float* orow = out + (active ? row : 0) * ldo;
        __syncthreads();
        double s = 0.0;
        for (int j = gid; j < d; j += G) {
            const float v = clamp1(xr[j], q);
            if (COLS > 0) held[g][j] = v;
            s += (double)v * (double)v;
        }
        s = wave_sum_f64(s);
        if ((gid & 63) == 0) red[g][gid >> 6] = s;
        __syncthreads();
        double tot = 0.0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) tot += red[g][w];
        const double nrm = sqrt(tot);
        const float den = (float)(nrm > 1e-12 ? nrm : (nrm != nrm ? nrm : 1e-12));
        if (active)
            for (int j = gid; j < d; j += G) orow[j] = (COLS > 0 ? held[g][j] : clamp1(xr[j], q)) / den;
    }
}

// a wave per row: hit = the row's m entries contain the row's own index; integer block sums.  ld = 0: every row reads the same
// m entries (the share of indices found anywhere in one table)
__global__ __launch_bounds__(256) void acc_count(const int* __restrict__ knn, long long n, long long m, long long ld,
                                                 long long* __restrict__ partial) {
    __shared__ int hits[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long row_blocks = (n + 3) / 4;
    int mine = 0;
    for (long long rb = blockIdx.x; rb < row_blocks; rb += gridDim.x) {
        const long long row = rb * 4 + wave;
        bool hit = false;
        if (row < n) {
            const int* kr = knn + row * ld;
            for (long long j = lane; j < m; j += 64) hit |= (long long)kr[j] == row;
        }
        mine += __ballot(hit) != 0ull;
    }
    if (lane == 0) hits[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (long long)hits[0] + hits[1] + hits[2] + hits[3];
}

__global__ __launch_bounds__(256) void acc_final(const long long* __restrict__ partial, int nblocks, long long n, double* __restrict__ out) {
    __shared__ long long red[256];
    long long s = 0;
    for (int j = threadIdx.x; j < nblocks; j += 256) s += partial[j];
    s = block_reduce<256>(s, red, OpSum());
    if (threadIdx.x == 0) out[0] = (double)s / (double)n;
}

constexpr int ACC_MAX_BLOCKS = 4096, SELECT_MAX_BLOCKS = 65536, KTH_MAX_BLOCKS = 1024;     // a workgroup counts at most 2^40 / 1024 elements into its 32-bit LDS counters
inline unsigned capped(long long want, int cap) { return (unsigned)(want < 1 ? 1 : want > cap ? cap : want); }
inline long long quant_parts(long long n) { return (n + QUANT_CHUNK - 1) / QUANT_CHUNK; }
inline int acc_blocks(long long n) { return (int)capped((n + 3) / 4, ACC_MAX_BLOCKS); }
struct KthPlan { long long hist, state, total; };          // the four passes' 256-bin histograms, then the state they hand on
KthPlan kth_plan() {
    KthPlan p;
    ScratchLayout lay;
    p.hist = lay.take(4 * 256 * 8), p.state = lay.take(sizeof(KthState)), p.total = lay.end;
    return p;
}

}  // namespace

// ---- plan and launchers (validation is the caller's: umlh_ops.cpp) ----
extern "C" {

unsigned long long umlh_outlier_quantile_bytes(long long n) { return (unsigned long long)align_up(quant_parts(n) * 8); }
unsigned long long umlh_outlier_kth_bytes(void) { return (unsigned long long)kth_plan().total; }
unsigned long long umlh_outlier_accuracy_bytes(long long n) { return (unsigned long long)align_up((long long)acc_blocks(n) * 8); }

int umlh_outlier_launch_quantile(const float* x, long long n, int d, long long ld, int lo, int hi, double frac, float* lo_val,
                                 float* hi_val, float* quant, double* mean64, float* q_val, void* scratch, hipStream_t st) {
    if (d <= WAVE_COLS)
        hipLaunchKernelGGL((row_select<256, 4, WAVE_COLS>), dim3(capped((n + 3) / 4, SELECT_MAX_BLOCKS)), dim3(256), 0, st, x, n, d, ld,
                           lo, hi, frac, lo_val, hi_val, quant);
    else if (d <= LDS_COLS)
        hipLaunchKernelGGL((row_select<1024, 1, LDS_COLS>), dim3(capped(n, SELECT_MAX_BLOCKS)), dim3(1024), 0, st, x, n, d, ld, lo, hi,
                           frac, lo_val, hi_val, quant);
    else
        hipLaunchKernelGGL((row_select<1024, 1, 0>), dim3(capped(n, SELECT_MAX_BLOCKS)), dim3(1024), 0, st, x, n, d, ld, lo, hi, frac,
                           lo_val, hi_val, quant);
    const long long parts = quant_parts(n);
    double* partial = at<double>(scratch, 0);
    hipLaunchKernelGGL(quant_partial, dim3((unsigned)parts), dim3(256), 0, st, quant, n, partial);
    hipLaunchKernelGGL(quant_final, dim3(1), dim3(256), 0, st, partial, parts, n, mean64, q_val);
    return (int)hipGetLastError();
}

int umlh_outlier_launch_kth(const float* x, long long n, long long d, long long ld, long long k, float* out, void* scratch,
                            hipStream_t st) {
    const KthPlan p = kth_plan();
    hipError_t e = hipMemsetAsync(scratch, 0, (size_t)p.total, st);
    if (e != hipSuccess) return (int)e;
    const long long total = n * d;
    unsigned long long* gh = at<unsigned long long>(scratch, p.hist);
    KthState* ks = at<KthState>(scratch, p.state);
    const long long nvec = ld == d && (reinterpret_cast<uintptr_t>(x) & 15) == 0 ? total / 4 : 0;
    const dim3 grid(capped((total + 4 * KTH_THREADS - 1) / (4 * KTH_THREADS), KTH_MAX_BLOCKS)), block(KTH_THREADS);
    hipLaunchKernelGGL(kth_pass<0>, grid, block, 0, st, x, total, d, ld, nvec, (unsigned long long)k, gh, ks, out);
    hipLaunchKernelGGL(kth_pass<1>, grid, block, 0, st, x, total, d, ld, nvec, (unsigned long long)k, gh, ks, out);
    hipLaunchKernelGGL(kth_pass<2>, grid, block, 0, st, x, total, d, ld, nvec, (unsigned long long)k, gh, ks, out);
    hipLaunchKernelGGL(kth_pass<3>, grid, block, 0, st, x, total, d, ld, nvec, (unsigned long long)k, gh, ks, out);
    return (int)hipGetLastError();
}

int umlh_outlier_launch_clamp(const float* x, long long n, int d, long long ldx, const float* q_val, int normalize, float* out,
                              long long ldo, hipStream_t st) {
    if (!normalize) {
        const bool dense = ldx == d && ldo == d;
        const long long rows = dense ? 1 : n, cols = dense ? n * d : d;
        const bool vec = dense && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
        const long long nvec = vec ? cols / 4 : 0;
        const long long work = vec ? (nvec + 255) / 256 : rows * ((cols + 1023) / 1024);
        hipLaunchKernelGGL(clamp_flat, dim3(capped(work, 8192)), dim3(256), 0, st, x, rows, cols, dense ? cols : ldx, q_val, out,
                           dense ? cols : ldo, nvec);
    } else if (d <= WAVE_COLS) {
        hipLaunchKernelGGL((clamp_norm<256, 4, WAVE_COLS>), dim3(capped((n + 3) / 4, SELECT_MAX_BLOCKS)), dim3(256), 0, st, x, n, d, ldx,
                           q_val, out, ldo);
    } else if (d <= LDS_COLS) {
        hipLaunchKernelGGL((clamp_norm<1024, 1, LDS_COLS>), dim3(capped(n, SELECT_MAX_BLOCKS)), dim3(1024), 0, st, x, n, d, ldx, q_val,
                           out, ldo);
    } else {
        hipLaunchKernelGGL((clamp_norm<1024, 1, 0>), dim3(capped(n, SELECT_MAX_BLOCKS)), dim3(1024), 0, st, x, n, d, ldx, q_val, out, ldo);
    }
    return (int)hipGetLastError();
}

int umlh_outlier_launch_accuracy(const int* knn, long long n, long long m, long long ld, double* out, void* scratch, hipStream_t st) {
    const int nblocks = acc_blocks(n);
    long long* partial = at<long long>(scratch, 0);
    hipLaunchKernelGGL(acc_count, dim3((unsigned)nblocks), dim3(256), 0, st, knn, n, m, ld, partial);
    hipLaunchKernelGGL(acc_final, dim3(1), dim3(256), 0, st, partial, nblocks, n, out);
    return (int)hipGetLastError();
}

}  // extern "C"
