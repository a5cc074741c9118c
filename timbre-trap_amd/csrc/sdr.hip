// Signal-distortion ratio on the device (include/ttrap.h: tt_sdr_*), float64 throughout, no atomics.
//
//   r[l] = sum_n t[n] t[n+l],  b[l] = sum_n t[n] p[n+l]  (linear, zeros beyond the end),  l < L <= 512
//   Toeplitz(r / |t|^2) h = b / (|t| |p|)   by the Levinson recursion;   coh = b . h;   SDR = 10 log10(coh / (1 - coh))
//
// k_sdr_correlate: grid (chunks of SDR_CHUNK samples) x clips, 256 threads.  A workgroup walks its chunk in tiles of SDR_TILE samples:
// the tile of t and the tile of t, p extended by the SDR_LMAX - 1 sample halo are staged into LDS as doubles (the fp32 -> fp64 conversion
// happens once, on load; every product of two converted fp32 values is exact in float64).  Every wave covers all SDR_LMAX lags -- lane j
// owns the SDR_K adjacent lags j SDR_K .. j SDR_K + SDR_K - 1 -- over a quarter of the tile's samples, SDR_K samples per step: a step reads
// SDR_K new t and p values of the lane's window (2 SDR_K LDS reads; t[n] itself is lane 0's window, read with v_readfirstlane) for
// 2 SDR_K^2 multiply-adds.  The LDS rows are SDR_K doubles padded to SDR_K + 1: lanes read the same element of consecutive rows, a
// stride of 18 dwords, which spreads the lanes of a 64-bit read's lane group over distinct banks.  The four waves' sums are added in wave order and the chunk's 2 L + 1 sums go to its own
// scratch row; k_sdr_reduce adds the rows in ascending chunk order (bit-reproducible).
#include "common.h"
#include <math.h>

#define SDR_LMAX 512
#define SDR_K 8
#define SDR_TILE 2048
#define SDR_CHUNK 8192                          // = tt_sdr_chunk(); a multiple of SDR_TILE
#define SDR_MEAN_CHUNK 65536
#define SDR_ROWS ((SDR_TILE + SDR_LMAX) / SDR_K)   // LDS rows of SDR_K (+1 pad) doubles per staged signal

static_assert(SDR_LMAX == 64 * SDR_K, "one wave covers every lag");
static_assert(SDR_TILE % (8 * SDR_K) == 0 && SDR_CHUNK % SDR_TILE == 0, "tiles split evenly over four waves");

namespace {

__device__ __forceinline__ int sdr_pos(int i) { return i + (i >> 3); }     // sample index within the staged tile -> padded LDS index

__device__ __forceinline__ void sdr_load_row(const double* tl, const double* pl, int row, double (&wt)[SDR_K], double (&wp)[SDR_K]) {
#pragma unroll
    for (int i = 0; i < SDR_K; ++i) {
        wt[i] = tl[row * (SDR_K + 1) + i];
        wp[i] = pl[row * (SDR_K + 1) + i];
    }
}

__device__ __forceinline__ double sdr_lane0(double v) {                    // the wave's lane-0 value, as a scalar operand
    const long long b = __double_as_longlong(v);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// SDR_K samples n = nb .. nb + SDR_K - 1 against the lane's lags: lo = T[nb + l0 ..], hi = T[nb + l0 + SDR_K ..] (T = t for r, p for b).
// t[nb + j] itself is element j of lane 0's window (l0 = 0 there): no LDS read for it.
__device__ __forceinline__ void sdr_step(const double (&tlo)[SDR_K], const double (&plo)[SDR_K], const double (&thi)[SDR_K],
                                         const double (&phi)[SDR_K], double (&ar)[SDR_K], double (&ab)[SDR_K]) {
#pragma unroll
    for (int j = 0; j < SDR_K; ++j) {
        const double tn = sdr_lane0(tlo[j]);
#pragma unroll
        for (int i = 0; i < SDR_K; ++i) {
            ar[i] = fma(tn, i + j < SDR_K ? tlo[i + j] : thi[i + j - SDR_K], ar[i]);
            ab[i] = fma(tn, i + j < SDR_K ? plo[i + j] : phi[i + j - SDR_K], ab[i]);
        }
    }
}

__global__ __launch_bounds__(256) void k_sdr_correlate(const float* __restrict__ preds, const float* __restrict__ target, long N, int L,
                                                       const double* __restrict__ means, int nchunks, double* __restrict__ scratch) {
    __shared__ double tl[SDR_ROWS * (SDR_K + 1)];
    __shared__ double pl[SDR_ROWS * (SDR_K + 1)];
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long clip = blockIdx.y;
    const float* __restrict__ p = preds + clip * N;
    const float* __restrict__ t = target + clip * N;
    const double mp = means ? means[2 * clip] : 0.0, mt = means ? means[2 * clip + 1] : 0.0;
    const long c0 = (long)blockIdx.x * SDR_CHUNK;
    const long c1 = c0 + SDR_CHUNK < N ? c0 + SDR_CHUNK : N;

    double ar[SDR_K], ab[SDR_K], pp = 0.0;
#pragma unroll
    for (int i = 0; i < SDR_K; ++i) ar[i] = ab[i] = 0.0;

    for (long base = c0; base < c1; base += SDR_TILE) {
        __syncthreads();                                    // the previous tile has been read
        for (int i = tid; i < SDR_TILE + SDR_LMAX; i += 256) {
            const long n = base + i;
            double tv = 0.0, pv = 0.0;
            if (n < N) {
                tv = (double)t[n] - mt;
                pv = (double)p[n] - mp;
                if (i < SDR_TILE && n < c1) pp += pv * pv;
            }
            tl[sdr_pos(i)] = tv;
            pl[sdr_pos(i)] = pv;
        }
        __syncthreads();
        // this wave's samples of the tile: [n0, n1), cut at the chunk's end (samples beyond it are zeros: nothing to add)
        const int per_wave = SDR_TILE / 4;
        const int n0 = wave * per_wave;
        long left = c1 - base - n0;
        const int n1 = n0 + (int)(left < 0 ? 0 : (left < per_wave ? left : per_wave));
        // the window of SDR_K + (SDR_K - 1) values a step needs lives in two register halves that swap roles from step to step
        double wt0[SDR_K], wp0[SDR_K], wt1[SDR_K], wp1[SDR_K];
        sdr_load_row(tl, pl, n0 / SDR_K + lane, wt0, wp0);
        for (int nb = n0; nb < n1; nb += 2 * SDR_K) {       // rows read: <= (SDR_TILE - 2 SDR_K) / SDR_K + 63 + 2 = SDR_ROWS - 1
            sdr_load_row(tl, pl, nb / SDR_K + lane + 1, wt1, wp1);
            sdr_step(wt0, wp0, wt1, wp1, ar, ab);
            // steps come in pairs: where n1 cuts a pair, n1 is the clip's end and the samples behind it were staged as zeros
            sdr_load_row(tl, pl, nb / SDR_K + lane + 2, wt0, wp0);
            sdr_step(wt1, wp1, wt0, wp0, ar, ab);
        }
    }

    // the four waves' sums in wave order, through the (now free) tile buffers
    __syncthreads();
#pragma unroll
    for (int i = 0; i < SDR_K; ++i) {
        tl[wave * SDR_LMAX + lane * SDR_K + i] = ar[i];
        pl[wave * SDR_LMAX + lane * SDR_K + i] = ab[i];
    }
    pp = wave_sum_d(pp);
    if (lane == 0) red[wave] = pp;
    __syncthreads();
    double* __restrict__ out = scratch + (clip * nchunks + blockIdx.x) * (long)(2 * L + 1);
    for (int l = tid; l < L; l += 256) {
        out[l] = ((tl[l] + tl[SDR_LMAX + l]) + tl[2 * SDR_LMAX + l]) + tl[3 * SDR_LMAX + l];
        out[L + l] = ((pl[l] + pl[SDR_LMAX + l]) + pl[2 * SDR_LMAX + l]) + pl[3 * SDR_LMAX + l];
    }
    if (tid == 0) out[2 * L] = ((red[0] + red[1]) + red[2]) + red[3];
}

// rb[clip][col] = sum over the chunk rows in ascending order; one thread per column
__global__ __launch_bounds__(64) void k_sdr_reduce(const double* __restrict__ scratch, int nchunks, int ncols, double* __restrict__ rb) {
    const int col = blockIdx.x * 64 + threadIdx.x;
    if (col >= ncols) return;
    const long clip = blockIdx.y;
    const double* __restrict__ s = scratch + clip * nchunks * (long)ncols + col;
    double acc = 0.0;
    int c = 0;
    for (; c + 8 <= nchunks; c += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = s[(long)(c + u) * ncols];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; c < nchunks; ++c) acc += s[(long)c * ncols];
    rb[clip * ncols + col] = acc;
}

// per-clip sums of preds and target over chunks of SDR_MEAN_CHUNK samples: part[clip][chunk][2]
__global__ __launch_bounds__(256) void k_sdr_sum_partial(const float* __restrict__ preds, const float* __restrict__ target, long N,
                                                         int nchunks, double* __restrict__ part) {
    __shared__ double red[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long clip = blockIdx.y;
    const long c0 = (long)blockIdx.x * SDR_MEAN_CHUNK;
    const long c1 = c0 + SDR_MEAN_CHUNK < N ? c0 + SDR_MEAN_CHUNK : N;
    double sp = 0.0, st = 0.0;
    for (long n = c0 + tid; n < c1; n += 256) {
        sp += (double)preds[clip * N + n];
        st += (double)target[clip * N + n];
    }
    sp = wave_sum_d(sp);
    st = wave_sum_d(st);
    if (lane == 0) {
        red[2 * wave] = sp;
        red[2 * wave + 1] = st;
    }
    __syncthreads();
    if (tid < 2) part[(clip * nchunks + blockIdx.x) * 2 + tid] = ((red[tid] + red[2 + tid]) + red[4 + tid]) + red[6 + tid];
}

__global__ __launch_bounds__(64) void k_sdr_mean_finish(const double* __restrict__ part, long N, int nchunks, double* __restrict__ means) {
    const int tid = threadIdx.x;
    if (tid >= 2) return;
    const long clip = blockIdx.x;
    double acc = 0.0;
    for (int c = 0; c < nchunks; ++c) acc += part[(clip * nchunks + c) * 2 + tid];
    means[2 * clip + tid] = acc / (double)N;
}

// One wave per clip: normalise, then the Levinson recursion for Toeplitz(r) h = b.  r, b and a mirror of the prediction polynomial a
// are in LDS (the recursion reads r and a backwards: r[k-i], a[k-i]); element i of a and of the solution h also lives in a register
// of lane i & 63.  Step k, with E the prediction error (1 / E is carried: one division per step):
//     acc = sum_i a[i] r[k-i],  q = sum_i h[i] r[k-i]  (i <= k; a[k] = h[k] = 0 before the step)        ref = -acc / E
//     a'[i] = a[i] + ref a[k-i]        E' = E (1 - ref^2)        h'[i] = h[i] + (b[k] - q) / E' a'[k-i],  a'[k-i] = a[k-i] + ref a[i]
// L - 1 steps whatever the data: a singular system ends in a non-finite result, never in a loop.
__global__ __launch_bounds__(64) void k_sdr_finish(const double* __restrict__ rb, int L, double load_diag, int has_load_diag,
                                                   double* __restrict__ coh_out, double* __restrict__ sdr_out) {
    constexpr int J = SDR_LMAX / 64;
    __shared__ double r[SDR_LMAX], b[SDR_LMAX], am[SDR_LMAX];
    const int lane = threadIdx.x;
    const long clip = blockIdx.x;
    const double* __restrict__ in = rb + clip * (long)(2 * L + 1);
    const double nt = fmax(sqrt(in[0]), 1e-6), np = fmax(sqrt(in[2 * L]), 1e-6);
    for (int i = lane; i < SDR_LMAX; i += 64) {
        double rv = i < L ? in[i] / (nt * nt) : 0.0;
        if (i == 0 && has_load_diag) rv += load_diag;
        r[i] = rv;
        b[i] = i < L ? in[L + i] / (nt * np) : 0.0;
        am[i] = i == 0 ? 1.0 : 0.0;
    }
    __syncthreads();
    double a[J], h[J];
#pragma unroll
    for (int j = 0; j < J; ++j) a[j] = h[j] = 0.0;
    double E = r[0], invE = 1.0 / E;
    if (lane == 0) {
        a[0] = 1.0;
        h[0] = b[0] * invE;
    }
    for (int k = 1; k < L; ++k) {
        double rr[J], ar[J], acc = 0.0, q = 0.0;
        const double bk = b[k];
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int i = lane + 64 * j;
            rr[j] = ar[j] = 0.0;
            if (64 * j <= k && i <= k) {                     // the first test is uniform: whole rows beyond k cost nothing
                rr[j] = r[k - i];
                ar[j] = am[k - i];
            }
        }
#pragma unroll
        for (int j = 0; j < J; ++j) {
            acc = fma(a[j], rr[j], acc);
            q = fma(h[j], rr[j], q);
        }
        acc = wave_sum_d(acc);
        q = wave_sum_d(q);
        const double ref = -acc * invE;
        E *= 1.0 - ref * ref;
        invE = 1.0 / E;
        const double lambda = (bk - q) * invE;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int i = lane + 64 * j;
            if (64 * j <= k && i <= k) {
                const double an = fma(ref, ar[j], a[j]), arev = fma(ref, a[j], ar[j]);
                h[j] = fma(lambda, arev, h[j]);
                a[j] = an;
                am[i] = an;
            }
        }
        __syncthreads();                                    // the next step reads am backwards
    }
    double coh = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) coh = fma(b[lane + 64 * j], h[j], coh);
    coh = wave_sum_d(coh);
    if (lane == 0) {
        const double ratio = coh / (1.0 - coh);
        coh_out[clip] = coh;
        sdr_out[clip] = ratio > 0.0 ? 10.0 * log10(ratio) : (ratio != ratio ? ratio : -INFINITY);
    }
}

inline bool sdr_args_ok(int B, int64_t N, int L) { return B >= 1 && N >= 1 && L >= 1 && L <= SDR_LMAX; }
inline int64_t sdr_chunks(int64_t N) { return (N + SDR_CHUNK - 1) / SDR_CHUNK; }
inline int64_t sdr_mean_chunks(int64_t N) { return (N + SDR_MEAN_CHUNK - 1) / SDR_MEAN_CHUNK; }

}  // namespace

extern "C" int tt_sdr_chunk(void) { return SDR_CHUNK; }

extern "C" int64_t tt_sdr_scratch_bytes(int B, int64_t N, int L) {
    if (!sdr_args_ok(B, N, L)) return TT_E_BADARG;
    const int64_t corr = (int64_t)B * sdr_chunks(N) * (2 * L + 1), mean = (int64_t)B * sdr_mean_chunks(N) * 2;
    return (corr > mean ? corr : mean) * (int64_t)sizeof(double);
}

extern "C" int tt_sdr_means(const float* preds, const float* target, int B, int64_t N, void* scratch, double* means_out, void* stream) {
    if (!preds || !target || !scratch || !means_out || !sdr_args_ok(B, N, 1)) return TT_E_BADARG;
    const int64_t nc = sdr_mean_chunks(N);
    if (nc > 0x7fffffff || B > 65535) return TT_E_UNSUPPORTED;
    hipLaunchKernelGGL(k_sdr_sum_partial, dim3((unsigned)nc, B), dim3(256), 0, tt_stream(stream), preds, target, (long)N, (int)nc,
                       (double*)scratch);
    TT_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sdr_mean_finish, dim3(B), dim3(64), 0, tt_stream(stream), (const double*)scratch, (long)N, (int)nc, means_out);
    TT_LAUNCH_CHECK();
    return 0;
}

extern "C" int tt_sdr_correlate(const float* preds, const float* target, int B, int64_t N, int L, const double* means, void* scratch,
                                double* rb_out, void* stream) {
    if (!preds || !target || !scratch || !rb_out || !sdr_args_ok(B, N, L)) return TT_E_BADARG;
    const int64_t nc = sdr_chunks(N);
    if (nc > 0x7fffffff || B > 65535) return TT_E_UNSUPPORTED;
    hipLaunchKernelGGL(k_sdr_correlate, dim3((unsigned)nc, B), dim3(256), 0, tt_stream(stream), preds, target, (long)N, L, means, (int)nc,
                       (double*)scratch);
    TT_LAUNCH_CHECK();
    const int ncols = 2 * L + 1;
    hipLaunchKernelGGL(k_sdr_reduce, dim3((ncols + 63) / 64, B), dim3(64), 0, tt_stream(stream), (const double*)scratch, (int)nc, ncols,
                       rb_out);
    TT_LAUNCH_CHECK();
    return 0;
}

extern "C" int tt_sdr_finish(const double* rb, int B, int L, double load_diag, int has_load_diag, double* coh_out, double* sdr_out,
                             void* stream) {
    if (!rb || !coh_out || !sdr_out || !sdr_args_ok(B, 1, L)) return TT_E_BADARG;
    hipLaunchKernelGGL(k_sdr_finish, dim3(B), dim3(64), 0, tt_stream(stream), rb, L, load_diag, has_load_diag, coh_out, sdr_out);
    TT_LAUNCH_CHECK();
    return 0;
}
