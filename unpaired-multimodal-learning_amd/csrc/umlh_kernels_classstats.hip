// Class-grouped statistics of a feature matrix for the feature capture of the fine-tune loop (reference:
// vision_language/finetune.py:222-231) for gfx950: a stable counting sort of the rows by label, then per class the mean row
// and the mean distance of the class's rows to it.
//
// Class index (runs once per run; rows are cut into blocks of 256):
//   ci_count     one workgroup per block: labels into LDS (-1 where outside [0, n_class)); the LAST row of each label in the
//                block stores that label's count into counts[block][label] (zeroed before), so no atomics are needed.
//   ci_scan      one thread per class walks the blocks: counts[block][c] becomes the number of rows of c in earlier blocks,
//                total[c] the class size.
//   ci_offsets   one workgroup: exclusive sum of total[] into offsets[0 .. n_class].
//   ci_scatter   one workgroup per block: a row's slot is offsets[c] + counts[block][c] + (rows of c before it in the block).
//
// Class statistics.  A class is read through the range [mono[c], mono[c + 1]) of `order`, mono[] being the running maximum
// of offsets[] clamped to [0, n]: ranges are disjoint whatever offsets[] holds.  Entries of `order` outside [0, n) are skipped
// and do not count.  A range is cut into chunks of 256 entries; wave w of a workgroup takes the entries w, w + 4, ... of a
// chunk in ascending order, lanes stride the columns.
//   cs_plan      one workgroup: mono[], and slot0[c] = the first partial-sum slot of a class of more than one chunk.
//   cs_pass1     workgroups [0, n_class) run cs_small, workgroups n_class + s run cs_big_sum for chunk slot s.
//   cs_small     one workgroup per class of at most one chunk: column sums (fp64, four wave partials added in wave order),
//                mean = (float)(sum / count), written; then per row sum_j (x_j - mean_j)^2 in fp64 from the mean just
//                written (lanes stride columns, butterfly), fp64 sqrt, the rows added per wave, the waves in wave order.
//                The rows come back from L2 / L1: a class is read twice by the same workgroup, back to back.
//   cs_big_sum / cs_big_mean / cs_big_dist   the same two passes for a class of several chunks, one workgroup per chunk, the
//                chunk partials added in chunk order: a class holding every row is spread over n / 256 workgroups.
//   cs_final     one workgroup: dist[] of the several-chunk classes, then out2 = {sum_c dist[c] / n_class, empty classes}:
//                thread t adds the classes t, t + 1024, ... in ascending order, then a fixed tree over the 1024 partials.
//
// No float atomics, no grid barrier, no host read.  Every summation order is fixed by the arguments alone, and the 16-byte
// and 4-byte load paths add each column's rows in the same order: results are bitwise the same on both.
#include <climits>

#include "umlh_common.h"
#include "umlh_launch.h"

namespace {

constexpr int CS_CHUNK = 256;             // entries of `order` per chunk, rows per block of the index
constexpr int CS_WAVES = 4;
constexpr int CS_COLS = 1024;             // columns per pass of the column sums: 16 fp64 accumulators per lane
constexpr int CS_SCAN = 1024;             // threads of the single-workgroup kernels

// inclusive scan over the workgroup (CS_SCAN threads) in LDS; MAX: running maximum, else running sum
template <bool MAX>
__device__ __forceinline__ long long cs_block_scan(long long v, long long* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int s = 1; s < CS_SCAN; s <<= 1) {
        const long long o = t >= s ? sh[t - s] : (MAX ? LLONG_MIN : 0);
        __syncthreads();
        if (t >= s) sh[t] = MAX ? (sh[t] > o ? sh[t] : o) : sh[t] + o;
        __syncthreads();
    }
    return sh[t];
}

// ------------------------------------------------------------------ class index ------------------------------------------------------------------

__device__ __forceinline__ int ci_label(const long long* __restrict__ labels, long long i, long long n, int n_class) {
    if (i >= n) return -1;
    const long long l = labels[i];
    return l >= 0 && l < n_class ? (int)l : -1;
}

__global__ __launch_bounds__(CS_CHUNK) void ci_count(const long long* __restrict__ labels, long long n, int n_class,
                                                     int* __restrict__ counts) {
    __shared__ int lab[CS_CHUNK];
    const int t = threadIdx.x;
    const int mine = ci_label(labels, (long long)blockIdx.x * CS_CHUNK + t, n, n_class);
    lab[t] = mine;
    __syncthreads();
    if (mine < 0) return;
    int same = 1;
    for (int j = 0; j < t; ++j) same += lab[j] == mine;
    bool last = true;
    for (int j = t + 1; j < CS_CHUNK; ++j) last = last && lab[j] != mine;
    if (last) counts[(long long)blockIdx.x * n_class + mine] = same;
}

__global__ __launch_bounds__(256) void ci_scan(int* __restrict__ counts, int blocks, int n_class, int* __restrict__ total) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_class) return;
    int run = 0;
    for (int g = 0; g < blocks; ++g) {
        const long long at = (long long)g * n_class + c;
        const int k = counts[at];
        counts[at] = run;
        run += k;
    }
    total[c] = run;
}

__global__ __launch_bounds__(CS_SCAN) void ci_offsets(const int* __restrict__ total, int n_class, long long* __restrict__ offsets) {
    __shared__ long long sh[CS_SCAN];
    long long carry = 0;
    for (int base = 0; base < n_class; base += CS_SCAN) {
        const int c = base + (int)threadIdx.x;
        const long long v = c < n_class ? total[c] : 0;
        const long long inc = cs_block_scan<false>(v, sh);
        if (c < n_class) offsets[c] = carry + inc - v;
        carry += sh[CS_SCAN - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) offsets[n_class] = carry;
}

__global__ __launch_bounds__(CS_CHUNK) void ci_scatter(const long long* __restrict__ labels, long long n, int n_class,
                                                       const int* __restrict__ counts, const long long* __restrict__ offsets,
                                                       int* __restrict__ order) {
    __shared__ int lab[CS_CHUNK];
    const int t = threadIdx.x;
    const long long row = (long long)blockIdx.x * CS_CHUNK + t;
    const int mine = ci_label(labels, row, n, n_class);
    lab[t] = mine;
    __syncthreads();
    if (mine < 0) return;
    int before = 0;
    for (int j = 0; j < t; ++j) before += lab[j] == mine;
    const long long at = offsets[mine] + counts[(long long)blockIdx.x * n_class + mine] + before;
    if (at >= 0 && at < n) order[at] = (int)row;          // always true for the offsets ci_offsets wrote
}

// ---------------------------------------------------------------- class statistics ----------------------------------------------------------------

struct CsArgs {
    const float* feats;
    long long ld, n;
    int d, n_class;
    const int* order;
    const long long* offsets;
    float* means;
    long long ld_means;
    double* dist;
    double* out2;
    int* mono;        // [n_class + 1]
    int* slot0;       // [n_class + 1]
    int* ccount;      // [n_class]   valid rows of each class
    int* pcnt;        // [slots]
    double* pdist;    // [slots]
    double* psum;     // [slots][d]
    int slots;
};

__global__ __launch_bounds__(CS_SCAN) void cs_plan(const long long* __restrict__ offsets, long long n, int n_class,
                                                   int* __restrict__ mono, int* __restrict__ slot0) {
    __shared__ long long sh[CS_SCAN];
    long long carry = 0;
    for (int base = 0; base <= n_class; base += CS_SCAN) {
        const int c = base + (int)threadIdx.x;
        long long v = 0;
        if (c <= n_class) {
            v = offsets[c];
            v = v < 0 ? 0 : (v > n ? n : v);
        }
        long long inc = cs_block_scan<true>(v, sh);
        inc = inc > carry ? inc : carry;
        if (c <= n_class) mono[c] = (int)inc;
        const long long top = sh[CS_SCAN - 1];
        carry = top > carry ? top : carry;
        __syncthreads();
    }
    __syncthreads();                                      // mono[] of this workgroup's own stores is read below
    carry = 0;
    for (int base = 0; base < n_class; base += CS_SCAN) {
        const int c = base + (int)threadIdx.x;
        long long v = 0;
        if (c < n_class) {
            const int len = mono[c + 1] - mono[c];
            v = len > CS_CHUNK ? (len + CS_CHUNK - 1) / CS_CHUNK : 0;
        }
        const long long inc = cs_block_scan<false>(v, sh);
        if (c < n_class) slot0[c] = (int)(carry + inc - v);
        carry += sh[CS_SCAN - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) slot0[n_class] = (int)carry;
}

// The row this wave takes at its step `lane` of the chunk [r0, r1): entry r0 + wave + 4 lane of `order`, -1 when past the
// chunk or outside [0, n).
__device__ __forceinline__ int cs_wave_rows(const int* __restrict__ order, int r0, int r1, long long n, int wave, int lane) {
    const int p = r0 + wave + CS_WAVES * lane;
    if (p >= r1) return -1;
    const int r = order[p];
    return r >= 0 && r < n ? r : -1;
}

__device__ __forceinline__ int cs_wave_steps(int r0, int r1, int wave) {
    const int len = r1 - r0 - wave;
    return len <= 0 ? 0 : (len + CS_WAVES - 1) / CS_WAVES;
}

// Column sums of the chunk's valid rows over the columns [c0, c0 + CS_COLS): part[wave][col - c0] in LDS.
template <bool VEC>
__device__ __forceinline__ void cs_col_sums(const float* __restrict__ feats, long long ld, int d, int c0, int rows, int steps,
                                            double (*part)[CS_COLS], int wave, int lane) {
    double acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0;
    for (int s = 0; s < steps; ++s) {
        const int r = __builtin_amdgcn_readlane(rows, s);
        if (r < 0) continue;
        const float* x = feats + (long long)r * ld;
        if (VEC) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = c0 + j * 256 + lane * 4;
                if (c < d) {
                    const float4 v = *reinterpret_cast<const float4*>(x + c);
                    acc[j * 4 + 0] += (double)v.x;
                    acc[j * 4 + 1] += (double)v.y;
                    acc[j * 4 + 2] += (double)v.z;
                    acc[j * 4 + 3] += (double)v.w;
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int c = c0 + i * 64 + lane;
                if (c < d) acc[i] += (double)x[c];
            }
        }
    }
    if (VEC) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) part[wave][j * 256 + lane * 4 + e] = acc[j * 4 + e];
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) part[wave][i * 64 + lane] = acc[i];
    }
}

// Sum over the wave's valid rows of |x - mean|_2, the same value in every lane.
template <bool VEC>
__device__ __forceinline__ double cs_row_dists(const float* __restrict__ feats, long long ld, int d, const float* mean,
                                               int rows, int steps, int lane) {
    double acc = 0.0;
    for (int s = 0; s < steps; ++s) {
        const int r = __builtin_amdgcn_readlane(rows, s);
        if (r < 0) continue;
        const float* x = feats + (long long)r * ld;
        double q = 0.0;
        if (VEC) {
            for (int c = lane * 4; c < d; c += 256) {
                const float4 v = *reinterpret_cast<const float4*>(x + c);
                const float4 m = *reinterpret_cast<const float4*>(mean + c);
                const double a = (double)v.x - (double)m.x, b = (double)v.y - (double)m.y;
                const double e = (double)v.z - (double)m.z, f = (double)v.w - (double)m.w;
                q += a * a;
                q += b * b;
                q += e * e;
                q += f * f;
            }
        } else {
            // the 16-byte path's order: lane l owns the columns 4 l .. 4 l + 3 of every group of 256
            for (int c = lane * 4; c < d; c += 256)
                for (int e = 0; e < 4 && c + e < d; ++e) {
                    const double a = (double)x[c + e] - (double)mean[c + e];
                    q += a * a;
                }
        }
        acc += sqrt(wave_sum_f64(q));
    }
    return acc;
}

// Valid rows of the chunk, the same value in every thread (CS_WAVES waves).
__device__ __forceinline__ int cs_count_valid(int rows, int* wcnt, int wave, int lane) {
    const int mine = __popcll(__ballot(rows >= 0));
    if (lane == 0) wcnt[wave] = mine;
    __syncthreads();
    int cnt = 0;
#pragma unroll
    for (int w = 0; w < CS_WAVES; ++w) cnt += wcnt[w];
    return cnt;
}

template <bool VEC>
__device__ __forceinline__ void cs_small(const CsArgs& a, int c, double (*part)[CS_COLS], double* wsum, int* wcnt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = a.mono[c], r1 = a.mono[c + 1];
    if (r1 - r0 > CS_CHUNK) return;                        // several chunks: cs_big_*
    const int rows = cs_wave_rows(a.order, r0, r1, a.n, wave, lane);
    const int steps = cs_wave_steps(r0, r1, wave);
    const int cnt = cs_count_valid(rows, wcnt, wave, lane);
    float* mean = a.means + (long long)c * a.ld_means;
    if (threadIdx.x == 0) a.ccount[c] = cnt;
    if (cnt == 0) {                                        // the mean of an empty slice
        for (int j = threadIdx.x; j < a.d; j += 64 * CS_WAVES) mean[j] = __builtin_nanf("");
        if (threadIdx.x == 0) a.dist[c] = __builtin_nan("");
        return;
    }
    for (int c0 = 0; c0 < a.d; c0 += CS_COLS) {
        cs_col_sums<VEC>(a.feats, a.ld, a.d, c0, rows, steps, part, wave, lane);
        __syncthreads();
        for (int j = threadIdx.x; j < CS_COLS && c0 + j < a.d; j += 64 * CS_WAVES) {
            double s = part[0][j];
#pragma unroll
            for (int w = 1; w < CS_WAVES; ++w) s += part[w][j];
            mean[c0 + j] = (float)(s / (double)cnt);
        }
        __syncthreads();
    }
    // the mean row was stored by this workgroup: visible to all its waves after the barrier above
    const double mine = cs_row_dists<VEC>(a.feats, a.ld, a.d, mean, rows, steps, lane);
    if (lane == 0) wsum[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wsum[0];
#pragma unroll
        for (int w = 1; w < CS_WAVES; ++w) s += wsum[w];
        a.dist[c] = s / (double)cnt;
    }
}

// (class, chunk) of partial-sum slot `slot`: the class with slot0[c] <= slot < slot0[c + 1]; false past the last slot.
__device__ __forceinline__ bool cs_slot_class(const int* __restrict__ slot0, int n_class, int slot, int* c_out, int* k_out) {
    if (slot >= slot0[n_class]) return false;
    int lo = 0, hi = n_class;                              // slot0[lo] <= slot < slot0[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (slot0[mid] <= slot) lo = mid; else hi = mid;
    }
    *c_out = lo;
    *k_out = slot - slot0[lo];
    return true;
}

template <bool VEC>
__device__ __forceinline__ void cs_big_sum(const CsArgs& a, int slot, double (*part)[CS_COLS], int* wcnt) {
    int c, k;
    if (!cs_slot_class(a.slot0, a.n_class, slot, &c, &k)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = a.mono[c] + k * CS_CHUNK, end = a.mono[c + 1], r1 = r0 + CS_CHUNK < end ? r0 + CS_CHUNK : end;
    const int rows = cs_wave_rows(a.order, r0, r1, a.n, wave, lane);
    const int steps = cs_wave_steps(r0, r1, wave);
    const int cnt = cs_count_valid(rows, wcnt, wave, lane);
    if (threadIdx.x == 0) a.pcnt[slot] = cnt;
    double* out = a.psum + (long long)slot * a.d;
    for (int c0 = 0; c0 < a.d; c0 += CS_COLS) {
        cs_col_sums<VEC>(a.feats, a.ld, a.d, c0, rows, steps, part, wave, lane);
        __syncthreads();
        for (int j = threadIdx.x; j < CS_COLS && c0 + j < a.d; j += 64 * CS_WAVES) {
            double s = part[0][j];
#pragma unroll
            for (int w = 1; w < CS_WAVES; ++w) s += part[w][j];
            out[c0 + j] = s;
        }
        __syncthreads();
    }
}

// Workgroups [0, n_class): the classes of at most one chunk, whole; workgroups n_class + s: the column sums of chunk slot s.
template <bool VEC>
__global__ __launch_bounds__(64 * CS_WAVES) void cs_pass1(CsArgs a) {
    __shared__ double part[CS_WAVES][CS_COLS];
    __shared__ double wsum[CS_WAVES];
    __shared__ int wcnt[CS_WAVES];
    if ((int)blockIdx.x < a.n_class) cs_small<VEC>(a, (int)blockIdx.x, part, wsum, wcnt);
    else cs_big_sum<VEC>(a, (int)blockIdx.x - a.n_class, part, wcnt);
}

__global__ __launch_bounds__(256) void cs_big_mean(CsArgs a) {
    int c, k;
    if (!cs_slot_class(a.slot0, a.n_class, blockIdx.x, &c, &k) || k != 0) return;
    const int s0 = a.slot0[c], s1 = a.slot0[c + 1];
    int cnt = 0;
    for (int s = s0; s < s1; ++s) cnt += a.pcnt[s];
    if (threadIdx.x == 0) a.ccount[c] = cnt;
    float* mean = a.means + (long long)c * a.ld_means;
    for (int j = threadIdx.x; j < a.d; j += 256) {
        double s = a.psum[(long long)s0 * a.d + j];
        for (int q = s0 + 1; q < s1; ++q) s += a.psum[(long long)q * a.d + j];
        mean[j] = cnt > 0 ? (float)(s / (double)cnt) : __builtin_nanf("");
    }
}

template <bool VEC>
__global__ __launch_bounds__(64 * CS_WAVES) void cs_big_dist(CsArgs a) {
    __shared__ double wsum[CS_WAVES];
    int c, k;
    if (!cs_slot_class(a.slot0, a.n_class, blockIdx.x, &c, &k)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = a.mono[c] + k * CS_CHUNK, end = a.mono[c + 1], r1 = r0 + CS_CHUNK < end ? r0 + CS_CHUNK : end;
    const int rows = cs_wave_rows(a.order, r0, r1, a.n, wave, lane);
    const int steps = cs_wave_steps(r0, r1, wave);
    const double mine = cs_row_dists<VEC>(a.feats, a.ld, a.d, a.means + (long long)c * a.ld_means, rows, steps, lane);
    if (lane == 0) wsum[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wsum[0];
#pragma unroll
        for (int w = 1; w < CS_WAVES; ++w) s += wsum[w];
        a.pdist[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(CS_SCAN) void cs_final(CsArgs a) {
    __shared__ double sum[CS_SCAN];
    __shared__ int empty[CS_SCAN];
    const int t = threadIdx.x;
    double s = 0.0;
    int e = 0;
    for (int c = t; c < a.n_class; c += CS_SCAN) {
        const int s0 = a.slot0[c], s1 = a.slot0[c + 1], cnt = a.ccount[c];
        double v;
        if (s1 > s0) {                                     // several chunks: the chunk sums in chunk order
            v = a.pdist[s0];
            for (int q = s0 + 1; q < s1; ++q) v += a.pdist[q];
            v = cnt > 0 ? v / (double)cnt : __builtin_nan("");
            a.dist[c] = v;
        } else {
            v = a.dist[c];
        }
        s += v;
        e += cnt == 0;
    }
    sum[t] = s;
    empty[t] = e;
    __syncthreads();
    for (int w = CS_SCAN / 2; w > 0; w >>= 1) {
        if (t < w) {
            sum[t] += sum[t + w];
            empty[t] += empty[t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        a.out2[0] = sum[0] / (double)a.n_class;
        a.out2[1] = (double)empty[0];
    }
}

inline long long ci_blocks(long long n) { return (n + CS_CHUNK - 1) / CS_CHUNK; }
inline long long cs_slots(long long n) { return 2 * n / CS_CHUNK; }     // sum over classes of more than one chunk of their chunks
inline bool cs_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

struct ClassIndexPlan { int blocks; long long cells, counts, totals, total; };     // the block-by-class count table, the class totals
ClassIndexPlan classindex_plan(long long n, int n_class) {
    ClassIndexPlan p;
    ScratchLayout lay;
    p.blocks = (int)ci_blocks(n), p.cells = (long long)p.blocks * n_class;
    p.counts = lay.take(p.cells * 4), p.totals = lay.take((long long)n_class * 4), p.total = lay.end;
    return p;
}

struct ClassStatsPlan { long long slots, mono, slot0, ccount, pcnt, pdist, psum, total; };
ClassStatsPlan classstats_plan(long long n, int d, int n_class) {
    ClassStatsPlan p;
    ScratchLayout lay;
    p.slots = cs_slots(n);
    p.mono = lay.take(((long long)n_class + 1) * 4), p.slot0 = lay.take(((long long)n_class + 1) * 4);
    p.ccount = lay.take((long long)n_class * 4), p.pcnt = lay.take((p.slots + 1) * 4);
    p.pdist = lay.take((p.slots + 1) * 8), p.psum = lay.take((p.slots * d + 1) * 8), p.total = lay.end;
    return p;
}

}  // namespace

extern "C" unsigned long long umlh_classindex_bytes(long long n, int n_class) {
    const ClassIndexPlan p = classindex_plan(n, n_class);
    if (p.cells > (1LL << 28)) return 0;                   // the block-by-class count table: at most 1 GiB
    return (unsigned long long)p.total;
}

extern "C" int umlh_classindex_launch(const long long* labels, long long n, int n_class, int* order, long long* offsets, void* scratch,
                                      hipStream_t st) {
    const ClassIndexPlan p = classindex_plan(n, n_class);
    int *counts = at<int>(scratch, p.counts), *total = at<int>(scratch, p.totals);
    if (hipError_t e = hipMemsetAsync(counts, 0, (size_t)p.cells * sizeof(int), st)) return (int)e;
    hipLaunchKernelGGL(ci_count, dim3((unsigned)p.blocks), dim3(CS_CHUNK), 0, st, labels, n, n_class, counts);
    hipLaunchKernelGGL(ci_scan, dim3((unsigned)((n_class + 255) / 256)), dim3(256), 0, st, counts, p.blocks, n_class, total);
    hipLaunchKernelGGL(ci_offsets, dim3(1), dim3(CS_SCAN), 0, st, (const int*)total, n_class, offsets);
    hipLaunchKernelGGL(ci_scatter, dim3((unsigned)p.blocks), dim3(CS_CHUNK), 0, st, labels, n, n_class, (const int*)counts,
                       (const long long*)offsets, order);
    return (int)hipGetLastError();
}

extern "C" unsigned long long umlh_classstats_bytes(long long n, int d, int n_class) {
    return (unsigned long long)classstats_plan(n, d, n_class).total;
}

extern "C" int umlh_classstats_launch(const float* feats, long long ld, long long n, int d, const int* order, const long long* offsets,
                                      int n_class, float* means, long long ld_means, double* dist, double* out2, void* scratch,
                                      hipStream_t st) {
    const ClassStatsPlan p = classstats_plan(n, d, n_class);
    CsArgs a;
    a.feats = feats, a.ld = ld, a.n = n, a.d = d, a.n_class = n_class, a.order = order, a.offsets = offsets;
    a.means = means, a.ld_means = ld_means, a.dist = dist, a.out2 = out2, a.slots = (int)p.slots;
    a.mono = at<int>(scratch, p.mono), a.slot0 = at<int>(scratch, p.slot0), a.ccount = at<int>(scratch, p.ccount);
    a.pcnt = at<int>(scratch, p.pcnt), a.pdist = at<double>(scratch, p.pdist), a.psum = at<double>(scratch, p.psum);
    const bool vec = d % 4 == 0 && ld % 4 == 0 && ld_means % 4 == 0 && cs_aligned16(feats) && cs_aligned16(means);
    const dim3 wg(64 * CS_WAVES);
    hipLaunchKernelGGL(cs_plan, dim3(1), dim3(CS_SCAN), 0, st, offsets, n, n_class, a.mono, a.slot0);
    const dim3 pass1((unsigned)(n_class + p.slots));
    if (vec) hipLaunchKernelGGL(cs_pass1<true>, pass1, wg, 0, st, a);
    else hipLaunchKernelGGL(cs_pass1<false>, pass1, wg, 0, st, a);
    if (p.slots > 0) {
        hipLaunchKernelGGL(cs_big_mean, dim3((unsigned)p.slots), dim3(256), 0, st, a);
        if (vec) hipLaunchKernelGGL(cs_big_dist<true>, dim3((unsigned)p.slots), wg, 0, st, a);
        else hipLaunchKernelGGL(cs_big_dist<false>, dim3((unsigned)p.slots), wg, 0, st, a);
    }
    hipLaunchKernelGGL(cs_final, dim3(1), dim3(CS_SCAN), 0, st, a);
    return (int)hipGetLastError();
}
