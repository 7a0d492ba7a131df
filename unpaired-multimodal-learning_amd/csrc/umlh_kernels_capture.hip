// The two device operations of the MultiBench embedding capture (reference: MultiBench/train.py:300-347,456-512) for gfx950:
// packing the valid rows of a block of padded sequences into a matrix, and the mean cosine of paired rows.
//
//   cap_compact<V>   one workgroup per (sequence b, row chunk): its row offset is the sum of the clamped lengths of the
//                    sequences before b (an integer sum over the workgroup), then a plain copy of the chunk's valid rows,
//                    V = uint4 (16-byte accesses: d, the three strides and both pointers are multiples of 16 bytes) or
//                    V = unsigned (4-byte accesses).  Words are moved as integers: NaN payloads and -0.0 survive.
//                    The workgroup (B - 1, chunk 0) writes rows_total.
//   cap_cos_rows     a wave per row, lanes striding the columns: a.b, |a|^2 and |b|^2 in three fp64 accumulators (the fp32
//                    products are exact there), a butterfly across the wave, cos = a.b / (max(|a|, eps) max(|b|, eps)).
//                    Wave w of workgroup g takes the rows 4 g + w, 4 g + w + 4 G, ... in ascending order (G workgroups, a
//                    function of n alone), and the workgroup's four sums are added in wave order into partial[g].
//   cap_cos_final    partial[0 .. G) added in index order: 64 lanes take 16 consecutive partials each, lane 0 adds the 64.
//
// No float atomics, no grid barrier, no host read.  Every summation order is fixed by the arguments alone.
#include "umlh_common.h"
#include "umlh_launch.h"

namespace {

constexpr int CAP_CHUNK_WORDS = 8192;     // 4-byte words one compaction workgroup moves (at least one row)
constexpr int CAP_COS_WAVES = 4;          // rows in flight per workgroup of the cosine
constexpr int CAP_COS_MAX_WG = 1024;      // most workgroups (and partial sums) of the cosine: 64 lanes x 16 in the final
constexpr int CAP_FINAL_PER_LANE = CAP_COS_MAX_WG / 64;

__device__ __forceinline__ long long cap_rows(const long long* __restrict__ lengths, int b, int T, int drop_last) {
    long long len = lengths ? lengths[b] : T;
    len = len < 0 ? 0 : (len > T ? T : len);
    len -= drop_last;
    return len < 0 ? 0 : len;
}

template <typename V>
__global__ __launch_bounds__(256) void cap_compact(const V* __restrict__ z, int T, int dv, long long ldb, long long ldt,
                                                   const long long* __restrict__ lengths, int drop_last, V* __restrict__ out,
                                                   long long ldo, long long out_rows, int rows_per_chunk,
                                                   long long* __restrict__ rows_total) {
    __shared__ long long red[256];
    const int b = blockIdx.y, tid = threadIdx.x;
    const bool last = b == (int)gridDim.y - 1 && blockIdx.x == 0;
    const long long mine = cap_rows(lengths, b, T, drop_last);
    const long long t0 = (long long)blockIdx.x * rows_per_chunk;
    if (t0 >= mine && !last) return;                       // uniform over the workgroup
    long long s = 0;
    for (int i = tid; i < b; i += 256) s += cap_rows(lengths, i, T, drop_last);
    const long long off = block_reduce<256>(s, red, OpSum());
    if (last && tid == 0) rows_total[0] = off + mine;
    long long nrows = mine - t0;
    if (nrows <= 0) return;
    if (nrows > rows_per_chunk) nrows = rows_per_chunk;
    if (off + t0 + nrows > out_rows) nrows = out_rows - off - t0;      // rows past the caller's matrix are not written
    if (nrows <= 0) return;
    const V* src = z + (long long)b * ldb + t0 * ldt;
    V* dst = out + (off + t0) * ldo;
    const unsigned words = (unsigned)nrows * (unsigned)dv, udv = (unsigned)dv;     // <= max(CAP_CHUNK_WORDS, d): 32-bit index arithmetic
    for (unsigned i = tid; i < words; i += 256) {
        const unsigned r = i / udv, c = i - r * udv;
        dst[(long long)r * ldo + c] = src[(long long)r * ldt + c];
    }
}

__global__ __launch_bounds__(64 * CAP_COS_WAVES) void cap_cos_rows(const float* __restrict__ a, long long lda,
                                                                    const float* __restrict__ b, long long ldb, long long n, int d,
                                                                    double eps, float* __restrict__ rows, double* __restrict__ partial) {
    __shared__ double wsum[CAP_COS_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long step = (long long)gridDim.x * CAP_COS_WAVES;
    double acc = 0.0;
    for (long long r = (long long)blockIdx.x * CAP_COS_WAVES + wave; r < n; r += step) {
        const float* pa = a + r * lda;
        const float* pb = b + r * ldb;
        double ab = 0.0, aa = 0.0, bb = 0.0;
#pragma unroll 4
        for (int c = lane; c < d; c += 64) {
            const double x = (double)pa[c], y = (double)pb[c];
            ab += x * y;
            aa += x * x;
            bb += y * y;
        }
        ab = wave_sum_f64(ab);
        aa = wave_sum_f64(aa);
        bb = wave_sum_f64(bb);
        const double na = sqrt(aa), nb = sqrt(bb);
        const double cos_r = ab / ((na > eps ? na : eps) * (nb > eps ? nb : eps));   // a NaN or Inf element makes a.b NaN or the
                                                                                      // quotient Inf / Inf: NaN either way, as in torch
        if (rows && lane == 0) rows[r] = (float)cos_r;
        acc += cos_r;
    }
    if (lane == 0) wsum[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wsum[0];
#pragma unroll
        for (int w = 1; w < CAP_COS_WAVES; ++w) s += wsum[w];
        partial[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(64) void cap_cos_final(const double* __restrict__ partial, int groups, long long n,
                                                    double* __restrict__ out2) {
    __shared__ double part[64];
    const int lane = threadIdx.x;
    double s = 0.0;
    for (int i = lane * CAP_FINAL_PER_LANE; i < (lane + 1) * CAP_FINAL_PER_LANE && i < groups; ++i) s += partial[i];
    part[lane] = s;
    __syncthreads();
    if (lane == 0) {
        double t = part[0];
        for (int i = 1; i < 64; ++i) t += part[i];
        out2[0] = t / (double)n;
        out2[1] = t;
    }
}

inline int cap_cos_groups(long long n) {
    const long long g = (n + CAP_COS_WAVES - 1) / CAP_COS_WAVES;
    return (int)(g < CAP_COS_MAX_WG ? g : CAP_COS_MAX_WG);
}

inline bool cap_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" unsigned long long umlh_capture_cosine_bytes(long long n) {
    return (unsigned long long)align_up((long long)cap_cos_groups(n) * 8);
}

extern "C" int umlh_capture_launch_compact(const float* z, int B, int T, int d, long long ldb, long long ldt, const long long* lengths,
                                           int drop_last, float* out, long long ldo, long long out_rows, long long* rows_total,
                                           hipStream_t st) {
    const bool vec = d % 4 == 0 && ldb % 4 == 0 && ldt % 4 == 0 && ldo % 4 == 0 && cap_aligned16(z) && cap_aligned16(out);
    const int rows_per_chunk = d >= CAP_CHUNK_WORDS ? 1 : (CAP_CHUNK_WORDS / d < T ? CAP_CHUNK_WORDS / d : T);
    const dim3 grid((unsigned)((T + rows_per_chunk - 1) / rows_per_chunk), (unsigned)B);
    if (vec)
        hipLaunchKernelGGL(cap_compact<uint4>, grid, dim3(256), 0, st, reinterpret_cast<const uint4*>(z), T, d / 4, ldb / 4, ldt / 4,
                           lengths, drop_last, reinterpret_cast<uint4*>(out), ldo / 4, out_rows, rows_per_chunk, rows_total);
    else
        hipLaunchKernelGGL(cap_compact<unsigned>, grid, dim3(256), 0, st, reinterpret_cast<const unsigned*>(z), T, d, ldb, ldt, lengths,
                           drop_last, reinterpret_cast<unsigned*>(out), ldo, out_rows, rows_per_chunk, rows_total);
    return (int)hipGetLastError();
}

extern "C" int umlh_capture_launch_cosine(const float* a, long long lda, const float* b, long long ldb, long long n, int d, double eps,
                                          double* out2, float* rows, void* scratch, hipStream_t st) {
    const int groups = cap_cos_groups(n);
    double* partial = at<double>(scratch, 0);
    hipLaunchKernelGGL(cap_cos_rows, dim3((unsigned)groups), dim3(64 * CAP_COS_WAVES), 0, st, a, lda, b, ldb, n, d, eps, rows, partial);
    hipLaunchKernelGGL(cap_cos_final, dim3(1), dim3(64), 0, st, (const double*)partial, groups, n, out2);
    return (int)hipGetLastError();
}
