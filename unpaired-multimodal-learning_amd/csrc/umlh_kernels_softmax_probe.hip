// The multinomial (softmax) logistic probe for gfx950: the `LogisticRegression(max_iter=200)` of the reference's probe factory
// (MultiBench/train.py:96-99) on labels with more than two classes, and the L-BFGS linear probe of cached features.
//
//   f(W) = sum_i (logsumexp_c z_ic - z_{i,y_i}) + (1 / (2C)) sum_{c, j < d} W_cj^2,   z_ic = W_c . [x_i, 1]
//
//   sp_build    X~ = [x | 1 | 0-pad] (row stride Dp = d + 1 rounded up to 4), standardised on load when statistics are given;
//               16-byte loads when x allows them, 4-byte loads otherwise (the same values either way)
//   (gemm_f32)  Z = X~ W^T, Z_p = X~ p^T, G = R^T X (the d feature columns) as split-K slabs: the project's fp32 GEMM, skipped by a device flag
//   sp_zacc     fresh logits: the partial products of X~ W^T over chunks of 128 columns are added up in double (an fp32 chain
//               over all d + 1 columns left the gradient at the optimum of the d = 512 case at 2^-22.2 rms of its term
//               magnitudes, through the residuals; the bound is 2^-23)
//   sp_rows     a wave per row: logits carried in double (fresh, or advanced by t Z_p), max, log-sum-exp, the
//               residual R = softmax - onehot as fp32, the row losses summed in double per row block
//   sp_rsum     the intercepts' gradient, the column sums of R, in double per row chunk (colsum_chunk of umlh_gram.h): the
//               ones column makes an fp32 chain add near-equal terms, whose roundings line up instead of cancelling (measured
//               at W = 0, where every residual off the label is 1 / K: 2^-19.4 of the term magnitudes at n = 2048)
//   sp_rmean    one block: the column sums' totals and their mean over the classes, which sp_grad takes out: the rows of R
//               sum to 0 up to their fp32 rounding, and nothing restores a common shift of the unpenalised intercepts
//   sp_grad     g = slabs summed in slab order + W / C (double, rounded once); y = g - g_old; max|g|, sum|g|, |W_pen|^2 per block
//   sp_dots     the new rows of the Gram matrix of [s_1..s_h, y_1..y_h, g]: partial dots per element block
//   sp_dir      one block: fixed-order totals, the stop tests, the Gram update, the two-loop recursion in coefficient space
//   sp_comb     p = the linear combination of the stored vectors; g_old = g; W.p and |p|^2 of the penalised block
//   sp_ls       a wave per row: the loss at the 14 step lengths 4, 2, 1, .., 2^-11 from Z and Z_p, one pass
//   sp_select   one block: the largest step with sufficient decrease, or the precision floor
//   sp_update   W += t p (fp32), s = the difference of the stored iterates
//
// A fit is a fixed train of launches in stream order; after `halt` is set every remaining launch (the GEMMs included) returns
// at its first instruction.  Every sum runs in double in a fixed order; nothing uses a float atomic, a grid barrier or a host
// read.  A label outside [0, K) is never used as an address: its row has a zero residual and no loss.
#include "umlh_common.h"
#include "umlh_gram.h"
#include "umlh_launch.h"
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

namespace {

constexpr int SP_LS = 14;                // step lengths of the line search: 4, 2, 1, 1/2, .., 2^-11 (4 and 2 without history only)
constexpr int SP_MAXH = 32;              // most (s, y) pairs
constexpr int SP_NB = 2 * SP_MAXH + 1;   // most basis vectors of the direction
constexpr int SP_EBLOCKS = 512;          // most workgroups of a pass over the coefficients
constexpr int SP_RBLOCKS = 1024;         // most workgroups of a pass over the rows
constexpr int SP_MAX_SLABS = 64;
constexpr int SP_GEMM_KIDS = 4096;       // reduction rows per slab that gemm_f32 stages row ids for
constexpr double SP_ARMIJO = 1e-4;
constexpr double SP_PAIR_TOL = 1e-12;

struct SpState {
    int halt;            // != 0: every later launch of this call returns at once
    int no_fresh;        // != 0: the next Z = X~ W^T launch is skipped (the logits are advanced by t Z_p)
    int iter;            // accepted steps
    int cnt, head;       // stored pairs; the ring slot the next pair goes to
    int have_step;       // the last slot accepted a step: this slot has a new (s, y) pair
    int want_fresh;      // the stop test held on advanced logits: decide on fresh ones
    int fresh_now;       // this slot's logits came from the GEMM
    int first;           // no history: the step lengths 4 and 2 are on offer
    int pad;
    double t, f, gtp, max_grad, sumabs, wpen;
    double rmean;        // the mean over the classes of the column sums of R (0 up to the residuals' fp32 rounding)
    double shift;        // what re-basing the objective on fresh logits has added to it so far (taken out of `objectives`)
    double c[SP_NB];                 // p in the basis [s | y | g]
    double B[SP_NB * SP_NB];         // the Gram matrix of the basis, by slot
};

struct SpArgs {
    const float* x;
    const int* y;
    const double* stats;
    long long n, L;                  // rows; K * Dp
    int d, ldx, D, Dp, K, Kp, ldc, h, nb, max_iter;
    double inv_c, gtol;
    int eblocks, rblocks, ns, cchunks, zchunk;       // zchunk: columns of X~ per partial product of fresh logits
    long long slab_stride;
    SpState* st;
    float* coef;
    float *xt, *z32, *r, *g, *gold, *p, *S, *Y, *slabs;
    double *zd, *losspart, *gpart, *rpart, *rtot, *dotpart, *combpart, *lspart;
    umlh_probe_record_t* rec;
    double* objectives;
};

__device__ __forceinline__ double sp_nanmax(double a, double b) { return (a != a || a > b) ? a : b; }

struct OpNanMax { __device__ double operator()(double a, double b) const { return sp_nanmax(a, b); } };

// basis vector j of the direction: s slots, y slots, the gradient
__device__ __forceinline__ const float* sp_basis(const SpArgs& a, int j) {
    return j < a.h ? a.S + (long long)j * a.L : (j < 2 * a.h ? a.Y + (long long)(j - a.h) * a.L : a.g);
}

// ---- X~ ----
__global__ __launch_bounds__(256) void sp_build(SpArgs a, int vec) {
    const int q = a.Dp / 4;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.n * q) return;
    const long long row = idx / q;
    const int j0 = 4 * (int)(idx - row * q);
    const float* src = a.x + row * a.ldx;
    float v[4];
    if (vec && j0 + 4 <= a.d) {
        const f32x4v t = *reinterpret_cast<const f32x4v*>(src + j0);
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = j0 + e < a.d ? src[j0 + e] : 0.f;
    }
    f32x4v o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int j = j0 + e;
        float u = v[e];
        if (j < a.d) {
            if (a.stats) u = (float)(((double)u - a.stats[j]) * (1.0 / a.stats[a.d + j]));
        } else {
            u = j == a.d ? 1.f : 0.f;
        }
        o[e] = u;
    }
    *reinterpret_cast<f32x4v*>(a.xt + row * a.Dp + j0) = o;
}

// W = 0 (init == 0), the record and the objectives' NaN fill; the state was zeroed by a memset
__global__ __launch_bounds__(256) void sp_init(SpArgs a, int init) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (!init && idx < a.L) {
        const int c = (int)(idx / a.Dp), j = (int)(idx - (long long)c * a.Dp);
        if (j < a.D) a.coef[(long long)c * a.ldc + j] = 0.f;
    }
    if (a.objectives && idx <= a.max_iter) a.objectives[idx] = __builtin_nan("");
    if (idx == 0 && a.rec) {
        a.rec->iterations = 0;
        a.rec->converged = 0;
        a.rec->max_grad = 0.0;
        a.rec->objective = 0.0;
    }
}

// ---- fresh logits: zd (+)= the partial product in z32 ----
__global__ __launch_bounds__(256) void sp_zacc(SpArgs a, int first) {
    const SpState* st = a.st;
    if (st->halt || st->no_fresh) return;
    const long long total = a.n * a.K;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const long long i = idx / a.K;
        const int c = (int)(idx - i * a.K);
        const double v = (double)a.z32[i * a.Kp + c];
        a.zd[idx] = first ? v : a.zd[idx] + v;
    }
}

// ---- rows: logits, residuals, loss ----
__global__ __launch_bounds__(256) void sp_rows(SpArgs a) {
    const SpState* st = a.st;
    if (st->halt) return;
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool fresh = !st->no_fresh, adv = !fresh && st->have_step;
    const double t = st->t;
    const long long rs = (long long)blockIdx.x * a.n / a.rblocks, re = (long long)(blockIdx.x + 1) * a.n / a.rblocks;
    double loss = 0.0;
    for (long long i = rs + wave; i < re; i += 4) {
        double* zd = a.zd + i * a.K;
        const float* z32 = a.z32 + i * a.Kp;
        float* r = a.r + i * a.Kp;
        const int lab = a.y[i];
        const bool ok = lab >= 0 && lab < a.K;
        double m = -DBL_MAX, zy = 0.0;
        for (int c = lane; c < a.K; c += 64) {
            double z = zd[c];
            if (adv) {
                z += t * (double)z32[c];
                zd[c] = z;
            }
            m = z > m ? z : m;
            if (c == lab) zy = z;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double v = __shfl_xor(m, o, 64);
            m = v > m ? v : m;
        }
        zy = wave_sum_f64(zy);
        double se = 0.0;
        for (int c = lane; c < a.K; c += 64) se += exp(zd[c] - m);
        se = wave_sum_f64(se);
        const double inv = 1.0 / se;
        for (int c = lane; c < a.K; c += 64) r[c] = ok ? (float)(exp(zd[c] - m) * inv - (c == lab ? 1.0 : 0.0)) : 0.f;
        if (ok) loss += log(se) + m - zy;
    }
    if (lane == 0) red[wave] = loss;
    __syncthreads();
    if (tid == 0) a.losspart[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// ---- column sums of R: the gradient of the intercepts ----
__global__ __launch_bounds__(256) void sp_rsum(SpArgs a) {
    if (a.st->halt) return;
    const float* r = a.r;
    const int ld = a.Kp;
    colsum_chunk([=](int c) { return [=](long long i) { return (double)r[i * ld + c]; }; }, a.K, a.n, a.cchunks, a.rpart);
}

__global__ __launch_bounds__(256) void sp_rmean(SpArgs a) {
    SpState* st = a.st;
    if (st->halt) return;
    __shared__ double red[256];
    double s = 0.0;
    for (int c = threadIdx.x; c < a.K; c += 256) {
        const double v = chunk_total(a.rpart, a.cchunks, a.K, c);
        a.rtot[c] = v;
        s += v;
    }
    s = block_reduce<256>(s, red, OpSum());
    if (threadIdx.x == 0) st->rmean = s / (double)a.K;
}

// ---- gradient from the slabs ----
__global__ __launch_bounds__(256) void sp_grad(SpArgs a) {
    const SpState* st = a.st;
    if (st->halt) return;
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const long long es = (long long)blockIdx.x * a.L / a.eblocks, ee = (long long)(blockIdx.x + 1) * a.L / a.eblocks;
    float* ynew = st->have_step ? a.Y + (long long)st->head * a.L : nullptr;
    double mg = 0.0, sa = 0.0, ww = 0.0;
    for (long long e = es + tid; e < ee; e += 256) {
        const int c = (int)(e / a.Dp), j = (int)(e - (long long)c * a.Dp);
        float gv = 0.f;
        if (j < a.D) {
            double v = 0.0;
            if (j < a.d) {
                for (int s = 0; s < a.ns; ++s) v += (double)a.slabs[s * a.slab_stride + e];
            } else {
                v = a.rtot[c] - st->rmean;
            }
            if (j < a.d) {
                const double w = (double)a.coef[(long long)c * a.ldc + j];
                v += a.inv_c * w;
                ww += w * w;
            }
            mg = sp_nanmax(fabs(v), mg);
            sa += fabs(v);
            gv = (float)v;
        }
        a.g[e] = gv;
        if (ynew) ynew[e] = gv - a.gold[e];
    }
    mg = block_reduce<256>(mg, red, OpNanMax());
    sa = block_reduce<256>(sa, red, OpSum());
    ww = block_reduce<256>(ww, red, OpSum());
    if (tid == 0) {
        a.gpart[blockIdx.x * 3 + 0] = mg;
        a.gpart[blockIdx.x * 3 + 1] = sa;
        a.gpart[blockIdx.x * 3 + 2] = ww;
    }
}

// Fixed-order totals of an evaluation: the loss, max|g|, sum|g|, |W_pen|^2 -> (f, max_grad, sumabs, wpen).  One block of 256;
// the fit's direction kernel and the evaluation's output kernel both call it, so the two agree bit for bit.
__device__ __forceinline__ void sp_totals(const SpArgs& a, double* red, double& f, double& mg, double& sa, double& ww) {
    const int tid = threadIdx.x;
    double l = 0.0;
    for (int b = tid; b < a.rblocks; b += 256) l += a.losspart[b];
    l = block_reduce<256>(l, red, OpSum());
    double m = 0.0, s = 0.0, w = 0.0;
    for (int b = tid; b < a.eblocks; b += 256) {
        m = sp_nanmax(a.gpart[b * 3 + 0], m);
        s += a.gpart[b * 3 + 1];
        w += a.gpart[b * 3 + 2];
    }
    mg = block_reduce<256>(m, red, OpNanMax());
    sa = block_reduce<256>(s, red, OpSum());
    ww = block_reduce<256>(w, red, OpSum());
    f = l + 0.5 * a.inv_c * ww;
}

__global__ __launch_bounds__(256) void sp_evalout(SpArgs a, double* objective, double* max_grad, float* grad, int ldg) {
    __shared__ double red[256];
    double f, mg, sa, ww;
    sp_totals(a, red, f, mg, sa, ww);
    if (threadIdx.x == 0) {
        if (objective) *objective = f;
        if (max_grad) *max_grad = mg;
    }
    if (grad)
        for (long long e = threadIdx.x; e < a.L; e += 256) {
            const int c = (int)(e / a.Dp), j = (int)(e - (long long)c * a.Dp);
            if (j < a.D) grad[(long long)c * ldg + j] = a.g[e];
        }
}

// ---- new Gram rows ----
// Row q / nb (0: the new s, 1: the new y, 2: g) against basis vector q % nb, over this block's elements: pair q goes to wave
// q % 4, lanes stride the elements, a fixed butterfly adds them.
__global__ __launch_bounds__(256) void sp_dots(SpArgs a) {
    const SpState* st = a.st;
    if (st->halt) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long es = (long long)blockIdx.x * a.L / a.eblocks, ee = (long long)(blockIdx.x + 1) * a.L / a.eblocks;
    const int head = st->head, q0 = st->have_step ? 0 : 2 * a.nb;
    for (int q = q0 + wave; q < 3 * a.nb; q += 4) {
        const int row = q / a.nb, col = q - row * a.nb;
        const float* u = row == 0 ? a.S + (long long)head * a.L : (row == 1 ? a.Y + (long long)head * a.L : a.g);
        const float* v = sp_basis(a, col);
        double s = 0.0;
        for (long long e = es + lane; e < ee; e += 64) s += (double)u[e] * (double)v[e];
        s = wave_sum_f64(s);
        if (lane == 0) a.dotpart[(long long)blockIdx.x * 3 * a.nb + q] = s;
    }
}

__device__ __forceinline__ void sp_record(const SpArgs& a, SpState* st, int converged, double f, double mg) {
    st->halt = 1;
    st->no_fresh = 1;
    a.rec->iterations = st->iter;
    a.rec->converged = converged;
    a.rec->max_grad = mg;
    a.rec->objective = f;
}

// One block.  Totals, stop tests, Gram update, two-loop recursion on coefficients (dots through the Gram matrix).
__global__ __launch_bounds__(256) void sp_dir(SpArgs a, int k) {
    SpState* st = a.st;
    if (st->halt) return;
    __shared__ double red[256];
    __shared__ double rows[3 * SP_NB];
    const int tid = threadIdx.x, nb = a.nb, h = a.h;
    double f, mg, sa, ww;
    sp_totals(a, red, f, mg, sa, ww);
    const int have = st->have_step;
    if (tid < 3 * nb && (have || tid >= 2 * nb)) {
        double s = 0.0;
        for (int b = 0; b < a.eblocks; ++b) s += a.dotpart[(long long)b * 3 * nb + tid];
        rows[tid] = s;
    }
    __syncthreads();
    if (tid != 0) return;
    const bool fresh = !st->no_fresh;
    st->fresh_now = fresh;
    if (fresh) {
        if (k > 0) st->shift += f - st->f;
        st->f = f;
    }
    if (k == 0 && a.objectives) a.objectives[0] = f;
    f = st->f;
    st->max_grad = mg;
    st->sumabs = sa;
    st->wpen = ww;
    if (mg != mg || f != f) { sp_record(a, st, 0, f, mg); return; }
    if (mg <= a.gtol) {
        if (fresh) { sp_record(a, st, 1, f, mg); return; }
        st->want_fresh = 1;
    }
    if (k == a.max_iter) { sp_record(a, st, 0, f, mg); return; }
    if (!(sa > 0.0)) { sp_record(a, st, 1, f, mg); return; }           // g = 0 exactly: nothing to follow
    double* B = st->B;
    int head = st->head, cnt = st->cnt;
    const int gi = 2 * h;
    for (int r = have ? 0 : 2; r < 3; ++r) {
        const int ri = r == 0 ? head : (r == 1 ? h + head : gi);
        for (int cj = 0; cj < nb; ++cj) {
            const double v = rows[r * nb + cj];
            B[ri * SP_NB + cj] = v;
            B[cj * SP_NB + ri] = v;
        }
    }
    if (have) {
        const double sy = B[head * SP_NB + h + head], ss = B[head * SP_NB + head], yy = B[(h + head) * SP_NB + h + head];
        if (sy > SP_PAIR_TOL * sqrt(ss * yy)) {
            head = (head + 1) % h;
            cnt = cnt < h ? cnt + 1 : h;
        } else if (cnt == h) {
            cnt = h - 1;             // the skipped pair's s overwrote the oldest pair's slot
        }
    }
    double* c = st->c;
    double alpha[SP_MAXH];
    double gtp = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int j = 0; j < nb; ++j) c[j] = 0.0;
        if (cnt == 0) {
            c[gi] = -1.0 / sa;
        } else {
            c[gi] = 1.0;
            for (int i = cnt - 1; i >= 0; --i) {               // newest first
                const int si = (head - cnt + i + 2 * h) % h, yi = h + si;
                double dot = 0.0;
                for (int j = 0; j < nb; ++j) dot += B[si * SP_NB + j] * c[j];
                alpha[i] = dot / B[si * SP_NB + yi];
                c[yi] -= alpha[i];
            }
            const int sn = (head - 1 + h) % h, yn = h + sn;
            const double gamma = B[sn * SP_NB + yn] / B[yn * SP_NB + yn];
            for (int j = 0; j < nb; ++j) c[j] *= gamma;
            for (int i = 0; i < cnt; ++i) {                     // oldest first
                const int si = (head - cnt + i + 2 * h) % h, yi = h + si;
                double dot = 0.0;
                for (int j = 0; j < nb; ++j) dot += B[yi * SP_NB + j] * c[j];
                c[si] += alpha[i] - dot / B[si * SP_NB + yi];
            }
            for (int j = 0; j < nb; ++j) c[j] = -c[j];
        }
        gtp = 0.0;
        for (int j = 0; j < nb; ++j) gtp += c[j] * B[gi * SP_NB + j];
        if (gtp < 0.0 || cnt == 0) break;
        cnt = 0;                                                // not a descent direction: drop the history
    }
    st->head = head;
    st->cnt = cnt;
    st->first = cnt == 0;
    st->gtp = gtp;
    if (!(gtp < 0.0)) sp_record(a, st, gtp == 0.0 ? 2 : 0, f, mg);     // a zero gradient (fresh or not): nothing to follow
}

// ---- p ----
__global__ __launch_bounds__(256) void sp_comb(SpArgs a) {
    const SpState* st = a.st;
    if (st->halt) return;
    __shared__ double red[256];
    __shared__ double cs[SP_NB];
    const int tid = threadIdx.x;
    if (tid < a.nb) cs[tid] = st->c[tid];
    __syncthreads();
    const long long es = (long long)blockIdx.x * a.L / a.eblocks, ee = (long long)(blockIdx.x + 1) * a.L / a.eblocks;
    double wp = 0.0, pp = 0.0;
    for (long long e = es + tid; e < ee; e += 256) {
        double v = 0.0;
        for (int j = 0; j < a.nb; ++j)
            if (cs[j] != 0.0) v += cs[j] * (double)sp_basis(a, j)[e];
        const float pv = (float)v;
        a.p[e] = pv;
        a.gold[e] = a.g[e];
        const int c = (int)(e / a.Dp), j = (int)(e - (long long)c * a.Dp);
        if (j < a.d) {
            wp += (double)a.coef[(long long)c * a.ldc + j] * (double)pv;
            pp += (double)pv * (double)pv;
        }
    }
    wp = block_reduce<256>(wp, red, OpSum());
    pp = block_reduce<256>(pp, red, OpSum());
    if (tid == 0) {
        a.combpart[blockIdx.x * 2 + 0] = wp;
        a.combpart[blockIdx.x * 2 + 1] = pp;
    }
}

// ---- line search ----
// loss_i(t) = log sum_c exp(z_c + t u_c - M(t)) + M(t) - (z_y + t u_y) with the bound M(t) = max z + t max u >= every
// exponent (t > 0): one pass serves all step lengths.  A sum that underflows to 0 (the bound is loose by more than 700) makes
// that step length unacceptable (+inf), never attractive.
__global__ __launch_bounds__(256) void sp_ls(SpArgs a) {
    const SpState* st = a.st;
    if (st->halt) return;
    __shared__ double red[4][SP_LS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long rs = (long long)blockIdx.x * a.n / a.rblocks, re = (long long)(blockIdx.x + 1) * a.n / a.rblocks;
    double loss[SP_LS];
#pragma unroll
    for (int j = 0; j < SP_LS; ++j) loss[j] = 0.0;
    for (long long i = rs + wave; i < re; i += 4) {
        const int lab = a.y[i];
        if (lab < 0 || lab >= a.K) continue;                    // (uniform over the wave)
        const double* zd = a.zd + i * a.K;
        const float* up = a.z32 + i * a.Kp;
        double zm = -DBL_MAX, um = -DBL_MAX, zy = 0.0, uy = 0.0;
        for (int c = lane; c < a.K; c += 64) {
            const double z = zd[c], u = (double)up[c];
            zm = z > zm ? z : zm;
            um = u > um ? u : um;
            if (c == lab) { zy = z; uy = u; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double v = __shfl_xor(zm, o, 64), w = __shfl_xor(um, o, 64);
            zm = v > zm ? v : zm;
            um = w > um ? w : um;
        }
        zy = wave_sum_f64(zy);
        uy = wave_sum_f64(uy);
        double se[SP_LS];
#pragma unroll
        for (int j = 0; j < SP_LS; ++j) se[j] = 0.0;
        for (int c = lane; c < a.K; c += 64) {
            const double z = zd[c] - zm, u = (double)up[c] - um;          // both <= 0
            double t = 4.0;
#pragma unroll
            for (int j = 0; j < SP_LS; ++j, t *= 0.5) se[j] += exp(z + t * u);
        }
        double t = 4.0;
#pragma unroll
        for (int j = 0; j < SP_LS; ++j, t *= 0.5) {
            const double s = wave_sum_f64(se[j]);
            const double l = log(s) + (zm + t * um) - (zy + t * uy);
            loss[j] += s == 0.0 ? (double)INFINITY : l;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < SP_LS; ++j) red[wave][j] = loss[j];
    }
    __syncthreads();
    if (tid < SP_LS) a.lspart[(long long)blockIdx.x * SP_LS + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

__global__ __launch_bounds__(256) void sp_select(SpArgs a, int k) {
    SpState* st = a.st;
    if (st->halt) return;
    __shared__ double red[256];
    __shared__ double loss[SP_LS];
    const int tid = threadIdx.x;
    double wp = 0.0, pp = 0.0;
    for (int b = tid; b < a.eblocks; b += 256) {
        wp += a.combpart[b * 2 + 0];
        pp += a.combpart[b * 2 + 1];
    }
    wp = block_reduce<256>(wp, red, OpSum());
    pp = block_reduce<256>(pp, red, OpSum());
    if (tid < SP_LS) {
        double s = 0.0;
        for (int b = 0; b < a.rblocks; ++b) s += a.lspart[(long long)b * SP_LS + tid];
        loss[tid] = s;
    }
    __syncthreads();
    if (tid != 0) return;
    const double f0 = st->f, gtp = st->gtp, ww = st->wpen;
    double t = 4.0, tsel = 0.0, fsel = f0;
    for (int j = 0; j < SP_LS; ++j, t *= 0.5) {
        if (t > 1.0 && !st->first) continue;
        const double fj = loss[j] + 0.5 * a.inv_c * (ww + 2.0 * t * wp + t * t * pp);
        if (fj <= f0 + SP_ARMIJO * t * gtp) { tsel = t; fsel = fj; break; }
    }
    st->t = tsel;
    if (tsel == 0.0) {
        if (st->fresh_now) { sp_record(a, st, 2, f0, st->max_grad); return; }     // the precision floor
        st->have_step = 0;               // decide on fresh logits
        st->want_fresh = 0;
        st->no_fresh = 0;
        return;
    }
    st->f = fsel;
    st->iter += 1;
    if (a.objectives) a.objectives[st->iter] = fsel - st->shift;
    st->have_step = 1;
    st->no_fresh = (st->want_fresh || k + 1 == a.max_iter) ? 0 : 1;
    st->want_fresh = 0;
}

__global__ __launch_bounds__(256) void sp_update(SpArgs a) {
    const SpState* st = a.st;
    if (st->halt || st->t == 0.0) return;
    const double t = st->t;
    float* s = a.S + (long long)st->head * a.L;
    const long long es = (long long)blockIdx.x * a.L / a.eblocks, ee = (long long)(blockIdx.x + 1) * a.L / a.eblocks;
    for (long long e = es + threadIdx.x; e < ee; e += 256) {
        const int c = (int)(e / a.Dp), j = (int)(e - (long long)c * a.Dp);
        float sv = 0.f;
        if (j < a.D) {
            float* w = a.coef + (long long)c * a.ldc + j;
            const float w0 = *w, w1 = (float)((double)w0 + t * (double)a.p[e]);
            *w = w1;
            sv = w1 - w0;
        }
        s[e] = sv;
    }
}

// ---- folding the scaler into raw-feature weights ----
// One wave per class: w_cj = W_cj / sigma_j, b_c = W_cd - sum_j W_cj mu_j / sigma_j in double (lanes stride j, fixed butterfly).
__global__ __launch_bounds__(256) void sp_fold(const float* __restrict__ coef, int ldc, int K, int d, const double* __restrict__ stats,
                                                float* __restrict__ w, int ldw, float* __restrict__ bias) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= K) return;
    const float* src = coef + (long long)c * ldc;
    double s = 0.0;
    for (int j = lane; j < d; j += 64) {
        const double v = stats ? (double)src[j] / stats[d + j] : (double)src[j];
        if (stats) s += v * stats[j];
        w[(long long)c * ldw + j] = (float)v;
    }
    s = wave_sum_f64(s);
    if (lane == 0) bias[c] = (float)((double)src[d] - s);
}

struct SpPlan {
    int Dp, Kp, eblocks, rblocks, ns, chunk, cchunks, zchunk;
    long long L, slab_stride;
    long long st, xt, z32, r, zd, g, slabs, losspart, gpart, rpart, rtot, gold, p, S, Y, dotpart, combpart, lspart, total;
};

SpPlan sp_plan(long long n, int d, int K, int fit, int history) {
    SpPlan p;
    const int D = d + 1;
    p.Dp = (D + 3) / 4 * 4;
    p.Kp = (K + 3) / 4 * 4;
    p.L = (long long)K * p.Dp;
    p.eblocks = (int)std::max<long long>(1, std::min<long long>(SP_EBLOCKS, (p.L + 1023) / 1024));
    p.rblocks = (int)std::max<long long>(1, std::min<long long>(SP_RBLOCKS, (n + 7) / 8));
    // G = R^T X~: enough slabs to fill the chip, few enough rows per slab for the GEMM's staged row ids
    const long long tiles = (long long)((K + 63) / 64) * ((d + 63) / 64);
    long long splits = std::max<long long>((512 + tiles - 1) / tiles, (n + SP_GEMM_KIDS - 1) / SP_GEMM_KIDS);
    splits = std::max<long long>(1, std::min<long long>(splits, std::min<long long>(SP_MAX_SLABS, (n + 255) / 256)));
    p.chunk = (int)(((n + splits - 1) / splits + KT - 1) / KT * KT);
    p.ns = (int)((n + p.chunk - 1) / p.chunk);
    p.slab_stride = p.L;
    p.cchunks = (int)std::max<long long>(1, std::min<long long>(64, n / 128));
    const int zparts = (D + 127) / 128;
    p.zchunk = ((D + zparts - 1) / zparts + 3) / 4 * 4;
    const int nb = 2 * history + 1;
    ScratchLayout lay;
    p.st = lay.take(sizeof(SpState));
    p.xt = lay.take(4LL * n * p.Dp);
    p.z32 = lay.take(4LL * n * p.Kp), p.r = lay.take(4LL * n * p.Kp);
    p.zd = lay.take(8LL * n * K);
    p.g = lay.take(4LL * p.L);
    p.slabs = lay.take(4LL * p.ns * p.L);
    p.losspart = lay.take(8LL * p.rblocks), p.gpart = lay.take(8LL * 3 * p.eblocks);
    p.rpart = lay.take(8LL * p.cchunks * K), p.rtot = lay.take(8LL * K);
    p.gold = p.p = p.S = p.Y = p.dotpart = p.combpart = p.lspart = 0;
    if (fit) {
        p.gold = lay.take(4LL * p.L), p.p = lay.take(4LL * p.L);
        p.S = lay.take(4LL * history * p.L), p.Y = lay.take(4LL * history * p.L);
        p.dotpart = lay.take(8LL * 3 * nb * p.eblocks);
        p.combpart = lay.take(8LL * 2 * p.eblocks);
        p.lspart = lay.take(8LL * SP_LS * p.rblocks);
    }
    p.total = lay.end;
    return p;
}

SpArgs sp_args(const SpPlan& p, const float* x, long long n, int d, int ldx, const int* y, const double* stats, int K, double c,
               float* coef, int ldc, int history, int max_iter, double gtol, void* scratch) {
    SpArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.y = y; a.stats = stats; a.n = n; a.L = p.L;
    a.d = d; a.ldx = ldx; a.D = d + 1; a.Dp = p.Dp; a.K = K; a.Kp = p.Kp; a.ldc = ldc; a.h = history; a.nb = 2 * history + 1;
    a.max_iter = max_iter; a.inv_c = 1.0 / c; a.gtol = gtol;
    a.eblocks = p.eblocks; a.rblocks = p.rblocks; a.ns = p.ns; a.cchunks = p.cchunks; a.zchunk = p.zchunk; a.slab_stride = p.slab_stride;
    a.st = at<SpState>(scratch, p.st);
    a.coef = coef;
    a.xt = at<float>(scratch, p.xt); a.z32 = at<float>(scratch, p.z32); a.r = at<float>(scratch, p.r);
    a.zd = at<double>(scratch, p.zd); a.g = at<float>(scratch, p.g); a.slabs = at<float>(scratch, p.slabs);
    a.losspart = at<double>(scratch, p.losspart); a.gpart = at<double>(scratch, p.gpart); a.rpart = at<double>(scratch, p.rpart); a.rtot = at<double>(scratch, p.rtot);
    a.gold = at<float>(scratch, p.gold); a.p = at<float>(scratch, p.p); a.S = at<float>(scratch, p.S); a.Y = at<float>(scratch, p.Y);
    a.dotpart = at<double>(scratch, p.dotpart); a.combpart = at<double>(scratch, p.combpart); a.lspart = at<double>(scratch, p.lspart);
    return a;
}

// out[m][n] = sum_k A(m,k) B(n,k) on the project's fp32 GEMM; `skip`: the device flag that turns the launch into a no-op
int sp_gemm(const float* A, int lda, int ta, const float* B, int ldb, int tb, float* out, int ldo, int M, int N, int K, int ns, int chunk,
            long long slab_stride, const int* skip, hipStream_t st) {
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = A; g.B = B; g.out = out; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldo = ldo;
    g.alpha = 1.f; g.k_switch = K; g.k_valid1 = K; g.k_chunk = chunk; g.slab_stride = slab_stride; g.skip = skip;
    return umlh_f32_launch_gemm(&g, ta, tb, ns, st);
}

int sp_launch_build(const SpArgs& a, hipStream_t st) {
    const int vec = a.ldx % 4 == 0 && (reinterpret_cast<uintptr_t>(a.x) & 15) == 0;
    const long long groups = a.n * (a.Dp / 4);
    hipLaunchKernelGGL(sp_build, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st, a, vec);
    return (int)hipGetLastError();
}

// the logits (fresh: from W), the residuals and the gradient at the coefficients: the evaluation both entry points share
int sp_launch_eval(const SpArgs& a, const SpPlan& p, const int* skip_z, const int* halt, hipStream_t st) {
    const unsigned zb = (unsigned)std::min<long long>(2048, (a.n * a.K + 255) / 256);
    for (int k0 = 0; k0 < a.D; k0 += a.zchunk) {
        const int kc = std::min(a.zchunk, a.D - k0);
        if (int e = sp_gemm(a.xt + k0, a.Dp, 0, a.coef + k0, a.ldc, 0, a.z32, a.Kp, (int)a.n, a.K, kc, 1, kc, 0, skip_z, st)) return e;
        hipLaunchKernelGGL(sp_zacc, dim3(zb), dim3(256), 0, st, a, k0 == 0 ? 1 : 0);
    }
    hipLaunchKernelGGL(sp_rows, dim3((unsigned)a.rblocks), dim3(256), 0, st, a);
    hipLaunchKernelGGL(sp_rsum, dim3((unsigned)((a.K + 63) / 64), (unsigned)a.cchunks), dim3(256), 0, st, a);
    hipLaunchKernelGGL(sp_rmean, dim3(1), dim3(256), 0, st, a);
    if (int e = sp_gemm(a.r, a.Kp, 1, a.xt, a.Dp, 1, a.slabs, a.Dp, a.K, a.d, (int)a.n, p.ns, p.chunk, p.slab_stride, halt, st)) return e;
    hipLaunchKernelGGL(sp_grad, dim3((unsigned)a.eblocks), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace

// ---- plans and launchers (validation is the caller's: umlh_ops.cpp) ----
extern "C" {

unsigned long long umlh_softmax_probe_bytes(long long n, int d, int n_class, int fit, int history) {
    return (unsigned long long)sp_plan(n, d, n_class, fit, history).total;
}

int umlh_softmax_probe_launch_eval(const float* x, long long n, int d, int ldx, const int* y, const double* stats, int n_class, double c,
                                   float* coef, int ldc, double* objective, float* grad, int ldg, double* max_grad, void* scratch,
                                   hipStream_t st) {
    const SpPlan p = sp_plan(n, d, n_class, 0, 1);
    const SpArgs a = sp_args(p, x, n, d, ldx, y, stats, n_class, c, coef, ldc, 1, 0, 0.0, scratch);
    if (hipError_t e = hipMemsetAsync(a.st, 0, sizeof(SpState), st)) return (int)e;
    if (int e = sp_launch_build(a, st)) return e;
    if (int e = sp_launch_eval(a, p, nullptr, nullptr, st)) return e;
    hipLaunchKernelGGL(sp_evalout, dim3(1), dim3(256), 0, st, a, objective, max_grad, grad, ldg);
    return (int)hipGetLastError();
}

int umlh_softmax_probe_launch_fit(const float* x, long long n, int d, int ldx, const int* y, const double* stats, int n_class, double c,
                                  int max_iter, int history, double gtol, int init, float* coef, int ldc, umlh_probe_record_t* rec,
                                  double* objectives, void* scratch, hipStream_t st) {
    const SpPlan p = sp_plan(n, d, n_class, 1, history);
    SpArgs a = sp_args(p, x, n, d, ldx, y, stats, n_class, c, coef, ldc, history, max_iter, gtol, scratch);
    a.rec = rec;
    a.objectives = objectives;
    if (hipError_t e = hipMemsetAsync(a.st, 0, sizeof(SpState), st)) return (int)e;
    if (hipError_t e = hipMemsetAsync(a.S, 0, 4ull * history * p.L, st)) return (int)e;
    if (hipError_t e = hipMemsetAsync(a.Y, 0, 4ull * history * p.L, st)) return (int)e;
    const long long ninit = std::max<long long>(p.L, max_iter + 1);
    hipLaunchKernelGGL(sp_init, dim3((unsigned)((ninit + 255) / 256)), dim3(256), 0, st, a, init);
    if (int e = sp_launch_build(a, st)) return e;
    const int* halt = &a.st->halt;
    const dim3 eb((unsigned)a.eblocks), rb((unsigned)a.rblocks), b256(256);
    for (int k = 0; k <= max_iter; ++k) {
        if (int e = sp_launch_eval(a, p, &a.st->no_fresh, halt, st)) return e;
        hipLaunchKernelGGL(sp_dots, eb, b256, 0, st, a);
        hipLaunchKernelGGL(sp_dir, dim3(1), b256, 0, st, a, k);
        if (k == max_iter) break;
        hipLaunchKernelGGL(sp_comb, eb, b256, 0, st, a);
        if (int e = sp_gemm(a.xt, a.Dp, 0, a.p, a.Dp, 0, a.z32, a.Kp, (int)n, n_class, a.D, 1, a.D, 0, halt, st)) return e;
        hipLaunchKernelGGL(sp_ls, rb, b256, 0, st, a);
        hipLaunchKernelGGL(sp_select, dim3(1), b256, 0, st, a, k);
        hipLaunchKernelGGL(sp_update, eb, b256, 0, st, a);
    }
    return (int)hipGetLastError();
}

int umlh_softmax_probe_launch_fold(const float* coef, int ldc, int n_class, int d, const double* stats, float* w, int ldw, float* bias,
                                   hipStream_t st) {
    hipLaunchKernelGGL(sp_fold, dim3((unsigned)((n_class + 3) / 4)), dim3(256), 0, st, coef, ldc, n_class, d, stats, w, ldw, bias);
    return (int)hipGetLastError();
}

}  // extern "C"
