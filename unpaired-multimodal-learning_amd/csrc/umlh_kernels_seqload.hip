// The device loader of the affect datasets (reference: MultiBench/datasets/affect/get_data.py:159-261,418-444) for gfx950: what
// the reference's Dataset.__getitem__ and collate_fn do per sample and per batch on the host, done once per table on the device,
// plus the one kernel of the step path.
//
//   sl_first_row     start[n] = row of the first element of x[n] ([T, D] fp32) with x != 0 (NaN counts, -0.0 does not), T when
//                    there is none: text.nonzero()[0][0] of get_data.py:209.  One workgroup per sample; a thread walks the flat
//                    [T * D] words tid, tid + 256, ... and stops at its first hit, the workgroup takes the minimum row.
//   sl_colsum        column sums (pass 0) / sums of squared deviations from the mean (pass 1) in double, per row chunk:
//                    colsum_chunk of umlh_gram.h, the core of the probe's scaler statistics, here with a 64-bit row stride
//   sl_stats_final   fixed-order sum of the chunks -> mean | population std (a zero std stays zero: the division below then gives
//                    what IEEE division gives, as the reference's numpy expression does)
//   sl_col_apply     out = (float)(((double)x - mean) / std): the reference's vision_norm (get_data.py:185-191)
//   sl_znorm         per (sample, column) over rows start..T-1, in place: mean and unbiased std in double (one chain of at most T
//                    terms each, t ascending), then (x - (float)mean) / (float)std in fp32 and nan_to_num (NaN -> 0,
//                    +-Inf -> +-FLT_MAX): get_data.py:223-226.  One thread per (sample, column): the result of a sample does not
//                    depend on n, on the grid or on the workgroup that handled it.
//   sl_gather_pad    THE STEP-PATH KERNEL: one launch builds a batch.  Workgroup (chunk, b, m) copies words of the trimmed
//                    sequence of sample ids[b] of source m -- contiguous in the source ([len, D_m] from row start) and in the
//                    destination (out_m[b], [t_out, D_m]) -- and zero-fills the rest of the block.  Dword accesses, coalesced on
//                    both sides: with D in {5, 20, 35, 74, 300, 371} the 16-byte phase of source and destination differs from
//                    sequence to sequence, and at ~2.6 MB per batch the launch, not the access width, bounds the kernel
//                    (DESIGN section 22).  Four independent loads per thread before the first store.
//
// No atomics on global memory, no grid barrier, no host read.  Every result is bitwise reproducible across calls and streams.
#include "umlh_common.h"
#include "umlh_gram.h"
#include "umlh_launch.h"
#include <algorithm>
#include <cfloat>
#include <cmath>

namespace {

constexpr int SL_STAT_CHUNKS = UMLH_COLSTAT_CHUNKS;   // row chunks of the column statistics (shared with umlh_kernels_tabular.hip)
constexpr int SL_WG_WORDS = 1024;         // words one workgroup of the gather moves per step (4 per thread)
constexpr int SL_MAX_CHUNKS = 64;         // most workgroups along one (sample, source) block of the gather

// a start outside 0..T never becomes an address
__device__ __forceinline__ int sl_start(const int* __restrict__ start, long long n, int T) {
    const int s = start[n];
    return s < 0 ? 0 : (s > T ? T : s);
}

__global__ __launch_bounds__(256) void sl_first_row(const float* __restrict__ x, int T, int D, int* __restrict__ start) {
    __shared__ int first;
    const int tid = threadIdx.x, total = T * D;
    const float* p = x + (long long)blockIdx.x * total;
    if (tid == 0) first = T;
    __syncthreads();
    for (int i = tid; i < total; i += 256) {
        if (p[i] != 0.0f) {                       // true for NaN, false for -0.0
            atomicMin(&first, i / D);             // LDS
            break;
        }
    }
    __syncthreads();
    if (tid == 0) start[blockIdx.x] = first;
}

__global__ __launch_bounds__(256) void sl_colsum(const float* __restrict__ x, long long rows, int d, long long ldx, int chunks,
                                                 const double* __restrict__ mean, double* __restrict__ partial) {
    colsum_chunk([=](int c) {
        const double m = mean ? mean[c] : 0.0;
        return [=](long long r) {
            const double v = (double)x[r * ldx + c] - m;
            return mean ? v * v : v;
        };
    }, d, rows, chunks, partial);
}

__global__ __launch_bounds__(256) void sl_stats_final(const double* __restrict__ partial, long long rows, int d, int chunks, int pass,
                                                      double* __restrict__ stats) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= d) return;
    const double s = chunk_total(partial, chunks, d, c);
    if (pass == 0) stats[c] = s / (double)rows;
    else stats[d + c] = sqrt(s / (double)rows);
}

__global__ __launch_bounds__(256) void sl_col_apply(const float* x, long long rows, int d, long long ldx, const double* __restrict__ stats,
                                                    float* out, long long ldo) {      // out may be x itself
    const long long total = rows * d;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long r = i / d;
        const int c = (int)(i - r * d);
        out[r * ldo + c] = (float)(((double)x[r * ldx + c] - stats[c]) / stats[d + c]);
    }
}

__device__ __forceinline__ float sl_nan_to_num(float v) {
    if (v != v) return 0.0f;
    if (v == INFINITY) return FLT_MAX;
    if (v == -INFINITY) return -FLT_MAX;
    return v;
}

__global__ __launch_bounds__(64) void sl_znorm(float* __restrict__ x, int T, int d, const int* __restrict__ start) {
    const int c = blockIdx.y * 64 + threadIdx.x;
    if (c >= d) return;
    const int s = sl_start(start, blockIdx.x, T), len = T - s;
    if (len < 1) return;
    float* p = x + ((long long)blockIdx.x * T + s) * d + c;
    double sum = 0.0;
    for (int t = 0; t < len; ++t) sum += (double)p[(long long)t * d];
    const double mean = sum / (double)len;
    double ss = 0.0;
    for (int t = 0; t < len; ++t) {
        const double v = (double)p[(long long)t * d] - mean;
        ss += v * v;
    }
    const double sd = sqrt(ss / (double)(len - 1));          // len = 1: 0 / 0 = NaN, every element becomes 0 below
    const float m32 = (float)mean, s32 = (float)sd;
    for (int t = 0; t < len; ++t) {
        float* q = p + (long long)t * d;
        *q = sl_nan_to_num((*q - m32) / s32);
    }
}

struct GatherArgs {
    const float* src[UMLH_SEQ_GATHER_MAX_SOURCES];
    float* out[UMLH_SEQ_GATHER_MAX_SOURCES];
    int d[UMLH_SEQ_GATHER_MAX_SOURCES];
};

__global__ __launch_bounds__(256) void sl_gather_pad(GatherArgs a, long long n, int T, const int* __restrict__ start,
                                                     const long long* __restrict__ ids, int t_out, long long* __restrict__ lengths) {
    const int b = blockIdx.y, m = blockIdx.z, tid = threadIdx.x;
    const long long id = ids[b];
    int len = 0;
    long long first = 0;                                      // first row of the trimmed sequence in the [n * T] rows of a source
    if (id >= 0 && id < n) {
        const int s = sl_start(start, id, T);
        len = T - s < t_out ? T - s : t_out;
        first = id * T + s;
    }
    if (m == 0 && blockIdx.x == 0 && tid == 0) lengths[b] = len;
    if (!a.src[m]) return;
    const int d = a.d[m];
    const long long total = (long long)t_out * d, copy = (long long)len * d;
    const float* __restrict__ src = a.src[m] + first * d;
    float* __restrict__ dst = a.out[m] + (long long)b * total;
    for (long long i0 = (long long)blockIdx.x * SL_WG_WORDS; i0 < total; i0 += (long long)gridDim.x * SL_WG_WORDS) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long i = i0 + j * 256 + tid;
            v[j] = i < copy ? src[i] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long i = i0 + j * 256 + tid;
            if (i < total) dst[i] = v[j];
        }
    }
}

// The time-series noise of the robustness test sets (reference: MultiBench/robustness/timeseries_robust.py) on one table:
// unit u (a sample, or with PER_STEP a row) shares one host draw eps[u] and one host draw keep[u].  A workgroup takes whole
// samples, block-strided, and streams each like sl_gather_pad: dword accesses, 2048 words per step, eight loads in flight per
// thread before the first store.  src and dst may be the same table: a word is read and written by the same thread.  The first
// nonzero row of the RESULT falls out of the same pass: a thread remembers its first flat index with a result != 0 (its indices
// ascend), the workgroup takes the LDS minimum, and min(flat index) / D is the minimum row.
// SL_PERTURB_LOADS, the dword loads in flight per thread, was measured at 4, 8, 16: 4 643 x 50 x 300 takes
// 165 / 150 / 139 us and 4 643 x 50 x 35, whose 1 750-word samples are shorter than a 16-load step, 22.4 / 22.4 / 24.7 us.
constexpr int SL_PERTURB_LOADS = 8;

template <bool PER_STEP>
__global__ __launch_bounds__(256) void sl_perturb(const float* src, long long n, int T, int D, const double* __restrict__ eps,
                                                  const unsigned char* __restrict__ keep, unsigned thresh, int drop_all,
                                                  unsigned long long seed, float* dst, int* __restrict__ start_out) {
    __shared__ unsigned first;
    const unsigned tid = threadIdx.x, total = (unsigned)T * (unsigned)D;
    for (long long s = blockIdx.x; s < n; s += gridDim.x) {
        if (tid == 0) first = total;
        __syncthreads();
        const long long base = s * (long long)total;
        const float* p = src + base;
        float* q = dst + base;
        double e = 0.0;
        bool kept = true;
        if (!PER_STEP) {
            if (eps) e = eps[s];
            if (keep) kept = keep[s] != 0;
        }
        unsigned mine = total;
        for (unsigned i0 = 0; i0 < total; i0 += 256 * SL_PERTURB_LOADS) {
            float v[SL_PERTURB_LOADS];
#pragma unroll
            for (int j = 0; j < SL_PERTURB_LOADS; ++j) {
                const unsigned i = i0 + j * 256 + tid;
                v[j] = i < total ? p[i] : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < SL_PERTURB_LOADS; ++j) {
                const unsigned i = i0 + j * 256 + tid;
                if (i >= total) continue;
                if (PER_STEP) {
                    const long long u = s * T + (long long)(i / (unsigned)D);
                    if (eps) e = eps[u];
                    if (keep) kept = keep[u] != 0;
                }
                float r = v[j];
                if (eps) r = (float)((double)r + e);              // one fp64 add, one rounding
                if (!kept) r = 0.0f;                              // an assignment: NaN, Inf and -x become +0.0
                if (drop_all || (thresh && !keep_elem(seed, (unsigned long long)(base + i), thresh))) r = 0.0f;
                q[i] = r;
                if (r != 0.0f && i < mine) mine = i;              // true for NaN, false for -0.0
            }
        }
        if (start_out) {
            if (mine < total) atomicMin(&first, mine);            // LDS
            __syncthreads();
            if (tid == 0) start_out[s] = first < total ? (int)(first / (unsigned)D) : T;
        }
        __syncthreads();                                          // `first` is reset by the next sample
    }
}

struct ColnormPlan { int chunks; long long partial, total; };

ColnormPlan colnorm_plan(long long rows, int d) {
    ColnormPlan p;
    ScratchLayout lay;
    p.chunks = (int)std::min<long long>(SL_STAT_CHUNKS, rows);
    p.partial = lay.take(8LL * p.chunks * d), p.total = lay.end;
    return p;
}

}  // namespace

// ---- plans and launchers (validation is the caller's: umlh_ops.cpp) ----
extern "C" {

unsigned long long umlh_seqload_colnorm_bytes(long long rows, int d) { return (unsigned long long)colnorm_plan(rows, d).total; }

int umlh_seqload_launch_first_row(const float* x, long long n, int T, int D, int* start, hipStream_t st) {
    hipLaunchKernelGGL(sl_first_row, dim3((unsigned)n), dim3(256), 0, st, x, T, D, start);
    return (int)hipGetLastError();
}

int umlh_seqload_launch_stats_final(const double* partial, long long rows, int d, int chunks, int pass, double* stats, hipStream_t st) {
    hipLaunchKernelGGL(sl_stats_final, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, st, partial, rows, d, chunks, pass, stats);
    return (int)hipGetLastError();
}

int umlh_seqload_launch_colnorm(const float* x, long long rows, int d, long long ldx, float* out, long long ldo, double* stats,
                                void* scratch, hipStream_t st) {
    const ColnormPlan p = colnorm_plan(rows, d);
    double* partial = at<double>(scratch, p.partial);
    const dim3 grid((unsigned)((d + 63) / 64), (unsigned)p.chunks);
    for (int pass = 0; pass < 2; ++pass) {                    // pass 1 reads the means pass 0 wrote
        hipLaunchKernelGGL(sl_colsum, grid, dim3(256), 0, st, x, rows, d, ldx, p.chunks, pass ? (const double*)stats : nullptr, partial);
        umlh_seqload_launch_stats_final(partial, rows, d, p.chunks, pass, stats, st);
    }
    const long long blocks = (rows * d + 255) / 256;
    hipLaunchKernelGGL(sl_col_apply, dim3((unsigned)std::min<long long>(blocks, 1 << 16)), dim3(256), 0, st, x, rows, d, ldx,
                       (const double*)stats, out, ldo);
    return (int)hipGetLastError();
}

int umlh_seqload_launch_znorm(float* x, long long n, int T, int d, const int* start, hipStream_t st) {
    hipLaunchKernelGGL(sl_znorm, dim3((unsigned)n, (unsigned)((d + 63) / 64)), dim3(64), 0, st, x, T, d, start);
    return (int)hipGetLastError();
}

int umlh_seqload_launch_gather_pad(const float* const* srcs, const int* dims, int n_src, long long n, int T, const int* start,
                                   const long long* ids, int B, int t_out, float* const* outs, long long* lengths, hipStream_t st) {
    GatherArgs a;
    int d_max = 1;
    for (int m = 0; m < UMLH_SEQ_GATHER_MAX_SOURCES; ++m) {
        const bool on = m < n_src && srcs[m];
        a.src[m] = on ? srcs[m] : nullptr;
        a.out[m] = on ? outs[m] : nullptr;
        a.d[m] = on ? dims[m] : 0;
        if (a.d[m] > d_max) d_max = a.d[m];
    }
    const long long chunks = ((long long)t_out * d_max + SL_WG_WORDS - 1) / SL_WG_WORDS;
    const dim3 grid((unsigned)std::min<long long>(chunks, SL_MAX_CHUNKS), (unsigned)B, UMLH_SEQ_GATHER_MAX_SOURCES);
    hipLaunchKernelGGL(sl_gather_pad, grid, dim3(256), 0, st, a, n, T, start, ids, t_out, lengths);
    return (int)hipGetLastError();
}

int umlh_seqload_launch_perturb(const float* src, long long n, int T, int D, int per_step, const double* eps, const unsigned char* keep,
                                float elem_p, unsigned long long seed, float* dst, int* start_out, hipStream_t st) {
    const unsigned thresh = elem_p < 1.f ? umlh_enc_drop_thresh(elem_p) : 0u;       // as umlh_dropout forms it; p = 1 drops all
    const int drop_all = elem_p >= 1.f;
    const dim3 grid((unsigned)std::min<long long>(n, 1 << 16));
    if (per_step) hipLaunchKernelGGL(sl_perturb<true>, grid, dim3(256), 0, st, src, n, T, D, eps, keep, thresh, drop_all, seed, dst, start_out);
    else hipLaunchKernelGGL(sl_perturb<false>, grid, dim3(256), 0, st, src, n, T, D, eps, keep, thresh, drop_all, seed, dst, start_out);
    return (int)hipGetLastError();
}

}  // extern "C"
