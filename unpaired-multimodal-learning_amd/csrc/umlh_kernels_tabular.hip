// The MIMIC loader (reference: MultiBench/datasets/mimic/get_data.py, MultiBench/robustness/tabular_robust.py) for gfx950: the
// three kernels the affect loader of umlh_kernels_seqload.hip does not have.
//
//   tab_colsum       the column sums of sl_colsum on a float OR double source whose non-finite elements count as +0.0
//                    (X[isinf] = 0; X[isnan] = 0 of get_data.py:38-41): colsum_chunk of umlh_gram.h per row chunk, the chunks
//                    summed in order by the final kernel of umlh_kernels_seqload.hip.  Same plan, same chain: on a finite
//                    float source the statistics are those of umlh_seq_column_standardize bit for bit.
//   tab_col_apply    out = (float)((clean(x) - mean) / std), the subtraction and the division in double
//   tab_rows_narrow  the tabular noise on rows of at most 64 columns, a thread per row: drop, then the carry chain in a register
//   tab_rows_wide    the same on wider rows, a wave per row: out[j] is the dropped value of the last column <= j that does not
//                    carry, so a 64-column chunk takes an inclusive prefix maximum over lane indices and one cross-lane read;
//                    a chunk whose leading columns all carry takes the previous chunk's last result.  A lane reads and writes
//                    only its own column of a chunk: in place is safe.
//   tab_gather       THE STEP-PATH KERNEL: workgroup (chunk, b, m) copies words of row ids[b] of source m, a dense
//                    [n, widths[m]] table, to row b of its block; as sl_gather_pad without the trim, with a width per source.
//
// Values move as 32-bit words wherever they are only moved: NaN payloads and -0.0 survive.  No atomics on global memory, no
// host read: every result is bitwise reproducible across calls and streams.
#include "umlh_common.h"
#include "umlh_gram.h"
#include "umlh_launch.h"
#include <algorithm>

namespace {

constexpr int TAB_WG_WORDS = 1024;        // words one workgroup of the gather moves per step (4 per thread)
constexpr int TAB_MAX_CHUNKS = 64;        // most workgroups along one row of the gather
constexpr int TAB_NARROW_MAX = 64;        // widest row of the thread-per-row kernel: a wave's worth of columns

template <class T>
__device__ __forceinline__ T tab_clean(T v) { return __builtin_isfinite(v) ? v : (T)0; }

template <class T>
__global__ __launch_bounds__(256) void tab_colsum(const T* __restrict__ x, long long rows, int d, long long ldx, int chunks,
                                                  const double* __restrict__ mean, double* __restrict__ partial) {
    colsum_chunk([=](int c) {
        const double m = mean ? mean[c] : 0.0;
        return [=](long long r) {
            const double v = (double)tab_clean(x[r * ldx + c]) - m;
            return mean ? v * v : v;
        };
    }, d, rows, chunks, partial);
}

template <class T>
__global__ __launch_bounds__(256) void tab_col_apply(const T* x, long long rows, int d, long long ldx, const double* __restrict__ stats,
                                                     float* out, long long ldo) {        // out may be a float x itself
    const long long total = rows * d;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long r = i / d;
        const int c = (int)(i - r * d);
        out[r * ldo + c] = (float)(((double)tab_clean(x[r * ldx + c]) - stats[c]) / stats[d + c]);
    }
}

// the decisions of element (i, j): a host mask where one is given, else the counter stream (thresh 0 and all 0: never)
struct TabDraws {
    const unsigned char* drop;            // [n, d]
    const unsigned char* carry;           // [n, d - 1]: entry j - 1 is column j's
    unsigned drop_thresh, carry_thresh;
    int drop_all, carry_all;
    unsigned long long seed;
};

__device__ __forceinline__ bool tab_drops(const TabDraws& w, long long i, int j, int d) {
    const long long e = i * d + j;
    if (w.drop) return w.drop[e] != 0;
    return w.drop_all || (w.drop_thresh && !keep_elem(w.seed, (unsigned long long)e, w.drop_thresh));
}

__device__ __forceinline__ bool tab_carries(const TabDraws& w, long long i, int j, int d) {      // 1 <= j < d
    if (w.carry) return w.carry[i * (d - 1) + (j - 1)] != 0;
    return w.carry_all || (w.carry_thresh && !keep_elem(w.seed + 1, (unsigned long long)(i * d + j), w.carry_thresh));
}

__global__ __launch_bounds__(256) void tab_rows_narrow(const unsigned* src, long long n, int d, long long lds, TabDraws w, unsigned* dst,
                                                       long long ldd) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const unsigned* p = src + i * lds;
        unsigned* q = dst + i * ldd;
        unsigned last = 0u;
        for (int j = 0; j < d; ++j) {
            const unsigned v = tab_drops(w, i, j, d) ? 0u : p[j];              // read before column j is written
            if (j == 0 || !tab_carries(w, i, j, d)) last = v;
            q[j] = last;
        }
    }
}

__global__ __launch_bounds__(256) void tab_rows_wide(const unsigned* src, long long n, int d, long long lds, TabDraws w, unsigned* dst,
                                                     long long ldd) {
    const int lane = threadIdx.x & 63;
    for (long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += (long long)gridDim.x * 4) {    // wave-uniform
        const unsigned* p = src + i * lds;
        unsigned* q = dst + i * ldd;
        unsigned prev = 0u;                                                     // the result of the column before this chunk
        for (int c0 = 0; c0 < d; c0 += 64) {
            const int j = c0 + lane;
            const bool in = j < d;
            const unsigned v = (in && !tab_drops(w, i, j, d)) ? p[j] : 0u;
            int from = (in && j > 0 && tab_carries(w, i, j, d)) ? -1 : lane;    // the lane whose value this column takes
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int up = __shfl_up(from, off);
                if (lane >= off && up > from) from = up;
            }
            const unsigned got = (unsigned)__shfl((int)v, from < 0 ? 0 : from);
            const unsigned r = from < 0 ? prev : got;
            if (in) q[j] = r;
            prev = (unsigned)__shfl((int)r, 63);
        }
    }
}

struct RowsGatherArgs {
    const unsigned* src[UMLH_SEQ_GATHER_MAX_SOURCES];
    unsigned* out[UMLH_SEQ_GATHER_MAX_SOURCES];
    int width[UMLH_SEQ_GATHER_MAX_SOURCES];
};

__global__ __launch_bounds__(256) void tab_gather(RowsGatherArgs a, long long n, const long long* __restrict__ ids) {
    const int b = blockIdx.y, m = blockIdx.z, tid = threadIdx.x;
    if (!a.src[m]) return;
    const long long id = ids[b];
    const bool live = id >= 0 && id < n;                                        // else a zero row; id never becomes an address
    const long long width = a.width[m];
    const unsigned* __restrict__ src = a.src[m] + (live ? id : 0) * width;
    unsigned* __restrict__ dst = a.out[m] + (long long)b * width;
    for (long long i0 = (long long)blockIdx.x * TAB_WG_WORDS; i0 < width; i0 += (long long)gridDim.x * TAB_WG_WORDS) {
        unsigned v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long i = i0 + k * 256 + tid;
            v[k] = (live && i < width) ? src[i] : 0u;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long i = i0 + k * 256 + tid;
            if (i < width) dst[i] = v[k];
        }
    }
}

template <class T>
int launch_standardize(const T* x, long long rows, int d, long long ldx, float* out, long long ldo, double* stats, void* scratch,
                       hipStream_t st) {
    // the plan of umlh_seqload_launch_colnorm: min(rows, UMLH_COLSTAT_CHUNKS) row chunks, one region of doubles
    const int chunks = (int)std::min<long long>(UMLH_COLSTAT_CHUNKS, rows);
    double* partial = at<double>(scratch, 0);
    const dim3 grid((unsigned)((d + 63) / 64), (unsigned)chunks);
    for (int pass = 0; pass < 2; ++pass) {                    // pass 1 reads the means pass 0 wrote
        hipLaunchKernelGGL(tab_colsum<T>, grid, dim3(256), 0, st, x, rows, d, ldx, chunks, pass ? (const double*)stats : nullptr, partial);
        const int rc = umlh_seqload_launch_stats_final(partial, rows, d, chunks, pass, stats, st);
        if (rc) return rc;
    }
    const long long blocks = (rows * d + 255) / 256;
    hipLaunchKernelGGL(tab_col_apply<T>, dim3((unsigned)std::min<long long>(blocks, 1 << 16)), dim3(256), 0, st, x, rows, d, ldx,
                       (const double*)stats, out, ldo);
    return (int)hipGetLastError();
}

}  // namespace

// ---- launchers (validation is the caller's: umlh_ops.cpp) ----
extern "C" {

int umlh_tab_launch_standardize(const void* x, int x_is_f64, long long rows, int d, long long ldx, float* out, long long ldo,
                                double* stats, void* scratch, hipStream_t st) {
    return x_is_f64 ? launch_standardize(static_cast<const double*>(x), rows, d, ldx, out, ldo, stats, scratch, st)
                    : launch_standardize(static_cast<const float*>(x), rows, d, ldx, out, ldo, stats, scratch, st);
}

int umlh_tab_launch_perturb(const float* src, long long n, int d, long long lds, const unsigned char* drop, const unsigned char* carry,
                            float p_drop, float p_carry, unsigned long long seed, float* dst, long long ldd, hipStream_t st) {
    TabDraws w;
    w.drop = drop, w.carry = carry, w.seed = seed;
    w.drop_thresh = p_drop < 1.f ? umlh_enc_drop_thresh(p_drop) : 0u;           // as umlh_dropout forms it; p = 1 takes all
    w.carry_thresh = p_carry < 1.f ? umlh_enc_drop_thresh(p_carry) : 0u;
    w.drop_all = p_drop >= 1.f, w.carry_all = p_carry >= 1.f;
    const unsigned* s = reinterpret_cast<const unsigned*>(src);
    unsigned* t = reinterpret_cast<unsigned*>(dst);
    if (d <= TAB_NARROW_MAX)
        hipLaunchKernelGGL(tab_rows_narrow, dim3((unsigned)std::min<long long>((n + 255) / 256, 1 << 16)), dim3(256), 0, st, s, n, d, lds,
                           w, t, ldd);
    else
        hipLaunchKernelGGL(tab_rows_wide, dim3((unsigned)std::min<long long>((n + 3) / 4, 1 << 16)), dim3(256), 0, st, s, n, d, lds, w, t,
                           ldd);
    return (int)hipGetLastError();
}

int umlh_tab_launch_gather(const float* const* srcs, const int* widths, int n_src, long long n, const long long* ids, int B,
                           float* const* outs, hipStream_t st) {
    RowsGatherArgs a;
    int w_max = 1;
    for (int m = 0; m < UMLH_SEQ_GATHER_MAX_SOURCES; ++m) {
        const bool on = m < n_src && srcs[m];
        a.src[m] = on ? reinterpret_cast<const unsigned*>(srcs[m]) : nullptr;
        a.out[m] = on ? reinterpret_cast<unsigned*>(outs[m]) : nullptr;
        a.width[m] = on ? widths[m] : 0;
        if (a.width[m] > w_max) w_max = a.width[m];
    }
    const long long chunks = ((long long)w_max + TAB_WG_WORDS - 1) / TAB_WG_WORDS;
    const dim3 grid((unsigned)std::min<long long>(chunks, TAB_MAX_CHUNKS), (unsigned)B, UMLH_SEQ_GATHER_MAX_SOURCES);
    hipLaunchKernelGGL(tab_gather, grid, dim3(256), 0, st, a, n, ids);
    return (int)hipGetLastError();
}

}  // extern "C"
