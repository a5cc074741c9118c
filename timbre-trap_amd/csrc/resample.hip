// Sample-rate conversion of whole tracks on the device (include/ttrap.h: tt_resample*), fp32, no atomics, bit-reproducible.
//
//   y[q new + p] = sum_{k < K} h[p][k] xz[q orig + k - w],   K = 2 w + orig,   xz = mono mix of x, zero beyond [0, L)
//
// the polyphase form of conv1d(pad(x, (w, w + orig)), h, stride = orig), transposed, flattened and cut to Lout = ceil(new L / orig)
// outputs.  Every output is one chain of K fused multiply-adds in ascending k.
//
// k_resample (the general case): a workgroup of four waves owns RS_TILE consecutive frames q of one clip.  It stages the
// RS_TILE orig + 2 w input samples those frames read into LDS once -- the mono mix (channels added in index order, then one IEEE
// divide by C) and the zero extension happen there, so the inner loop has no bounds checks -- and then walks the phases with LANES ALONG p:
// lane l of a phase block holds phase p = 64 block + l and RS_Q accumulators, one per frame of a sub-tile.  Per tap k it reads ht[k][p]
// (the tap table is passed TRANSPOSED, [K][new], so the 64 lanes read 256 contiguous bytes) and RS_Q samples xs[q orig + k], an address
// all lanes share (an LDS broadcast), for RS_Q multiply-adds.  The table (205 KB at 320:147, 589 KB at 320:441) does not fit the LDS; it is
// re-read by every workgroup and stays in L2.  The alternative -- lanes along k, one output per wave -- needs a 6-step wave
// reduction per output for 348 / 64 = 5.4 multiply-adds per lane, and leaves 36 of 384 lane slots idle at K = 348: more shuffles than
// arithmetic.  (phase block, sub-tile) items are dealt to the four waves round robin.
//
// k_resample_direct (new <= 4 and orig <= 8: 2:1, 1:2, 3:2): thread = output sample.  A workgroup owns RS_DIRECT_TILE frames, stages
// RS_DIRECT_TILE orig + 2 w samples and every thread walks its outputs; the few tap rows are read through the caches (at new = 1 the
// address is the same in every lane).
//
// Both kernels leave, when asked, the workgroup's max |y| over the outputs it stored in a slot of its own (peak_partials[clip][workgroup]).
// The maximum is taken on the bit patterns of |v|: non-negative floats order like their bits and a NaN (sign cleared) lies above
// +inf, so a NaN sample becomes the peak, as in torch's max, where fmaxf would drop it (the decode peak of csrc/cqt.hip does the same).
// k_resample_normalize forms the clip's peak from those slots and divides (IEEE divide, like torch's `/=`; this file is built
// without fast-math flags and must stay so).
#include "common.h"

#define RS_TILE 16                 // frames q per workgroup of k_resample (= tt_resample_tile())
#define RS_Q 8                     // frames per lane (accumulators); RS_TILE / RS_Q sub-tiles
#define RS_DIRECT_TILE 1024        // frames q per workgroup of k_resample_direct (= tt_resample_direct_tile())
#define RS_DIRECT_MAX_NEW 4
#define RS_DIRECT_MAX_ORIG 8
#define RS_MAX_TAPS 704            // K = 2 w + orig <= this: RS_TILE RS_MAX_TAPS floats of LDS (44 KiB) hold any staged tile
#define RS_MAX_PHASES 1024
#define RS_NORM_CHUNK 8192         // outputs per workgroup of k_resample_normalize

static_assert(RS_TILE % RS_Q == 0, "sub-tiles split the tile evenly");
static_assert(RS_TILE * RS_MAX_TAPS * 4 <= 65536, "the staged tile fits the default dynamic-LDS limit");
static_assert((RS_DIRECT_TILE * RS_DIRECT_MAX_ORIG + RS_MAX_TAPS) * 4 <= 65536, "so does the direct kernel's");

namespace {

__device__ __forceinline__ unsigned rs_absbits(float v) { return __float_as_uint(v) & 0x7fffffffu; }
__device__ __forceinline__ unsigned rs_umax(unsigned a, unsigned b) { return a > b ? a : b; }

__device__ __forceinline__ unsigned rs_wave_umax(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = rs_umax(v, (unsigned)__shfl_xor((int)v, o, 64));
    return v;
}

// the workgroup's maximum of `peak` (256 threads) -> *slot, by thread 0
__device__ __forceinline__ void rs_store_peak(unsigned peak, unsigned* red, float* slot) {
    const int tid = threadIdx.x;
    peak = rs_wave_umax(peak);
    if ((tid & 63) == 0) red[tid >> 6] = peak;
    __syncthreads();
    if (tid == 0) *slot = __uint_as_float(rs_umax(rs_umax(red[0], red[1]), rs_umax(red[2], red[3])));
}

// xs[i] = mono mix of x[clip][.][g0 + i], zero outside [0, L), for i < n
__device__ __forceinline__ void rs_stage(const float* __restrict__ x, int C, int64_t L, int64_t g0, int n, float* __restrict__ xs) {
    const float fc = (float)C;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int64_t g = g0 + i;
        float v = 0.f;
        if (g >= 0 && g < L) {
            v = x[g];
            for (int c = 1; c < C; ++c) v += x[(int64_t)c * L + g];
            v = v / fc;
        }
        xs[i] = v;
    }
}

__global__ __launch_bounds__(256) void k_resample(const float* __restrict__ x, int C, int64_t L, const float* __restrict__ ht, int orig,
                                                  int nnew, int width, float* __restrict__ y, int64_t Lout,
                                                  float* __restrict__ peak_partials) {
    extern __shared__ float xs[];                       // RS_TILE orig + 2 width samples, from q0 orig - width
    __shared__ unsigned red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t clip = blockIdx.y;
    const int64_t q0 = (int64_t)blockIdx.x * RS_TILE;
    const int K = 2 * width + orig;
    rs_stage(x + clip * C * L, C, L, q0 * orig - width, RS_TILE * orig + 2 * width, xs);
    __syncthreads();

    float* __restrict__ yc = y + clip * Lout;
    const int nblocks = (nnew + 63) >> 6;
    unsigned peak = 0u;
    for (int item = wave; item < nblocks * (RS_TILE / RS_Q); item += 4) {
        const int pb = item / (RS_TILE / RS_Q), sub = item - pb * (RS_TILE / RS_Q);
        const int p = pb * 64 + lane;
        const float* __restrict__ hp = ht + (p < nnew ? p : nnew - 1);     // idle lanes of the last block re-read the last phase
        const float* __restrict__ xq = xs + sub * RS_Q * orig;           // largest index read: (RS_TILE - 1) orig + K - 1
        float acc[RS_Q];
#pragma unroll
        for (int j = 0; j < RS_Q; ++j) acc[j] = 0.f;
#pragma unroll 4
        for (int k = 0; k < K; ++k) {
            const float h = hp[(int64_t)k * nnew];
#pragma unroll
            for (int j = 0; j < RS_Q; ++j) acc[j] = fmaf(h, xq[j * orig + k], acc[j]);
        }
        if (p < nnew) {
#pragma unroll
            for (int j = 0; j < RS_Q; ++j) {
                const int64_t n = (q0 + sub * RS_Q + j) * nnew + p;
                if (n < Lout) {
                    yc[n] = acc[j];
                    peak = rs_umax(peak, rs_absbits(acc[j]));
                }
            }
        }
    }
    if (peak_partials) rs_store_peak(peak, red, peak_partials + clip * gridDim.x + blockIdx.x);
}

template <int NEW>
__global__ __launch_bounds__(256) void k_resample_direct(const float* __restrict__ x, int C, int64_t L, const float* __restrict__ ht, int orig,
                                                         int width, float* __restrict__ y, int64_t Lout, float* __restrict__ peak_partials) {
    extern __shared__ float xs[];                       // RS_DIRECT_TILE orig + 2 width samples, from q0 orig - width
    __shared__ unsigned red[4];
    const int tid = threadIdx.x;
    const int64_t clip = blockIdx.y;
    const int64_t q0 = (int64_t)blockIdx.x * RS_DIRECT_TILE;
    const int K = 2 * width + orig;
    rs_stage(x + clip * C * L, C, L, q0 * orig - width, RS_DIRECT_TILE * orig + 2 * width, xs);
    __syncthreads();

    float* __restrict__ yc = y + clip * Lout;
    unsigned peak = 0u;
    for (int i = tid; i < RS_DIRECT_TILE * NEW; i += 256) {
        const int ql = i / NEW, p = i - ql * NEW;
        const int64_t n = q0 * NEW + i;
        if (n >= Lout) break;                           // n grows with i
        const float* __restrict__ xq = xs + ql * orig;  // largest index read: (RS_DIRECT_TILE - 1) orig + K - 1
        float acc = 0.f;
#pragma unroll 4
        for (int k = 0; k < K; ++k) acc = fmaf(ht[k * NEW + p], xq[k], acc);
        yc[n] = acc;
        peak = rs_umax(peak, rs_absbits(acc));
    }
    if (peak_partials) rs_store_peak(peak, red, peak_partials + clip * gridDim.x + blockIdx.x);
}

// y[clip][.] /= max over the clip's partials, unless that maximum is zero (a NaN peak is not zero: everything becomes NaN)
__global__ __launch_bounds__(256) void k_resample_normalize(float* __restrict__ y, int64_t Lout, const float* __restrict__ peak_partials,
                                                            int64_t n_partials) {
    __shared__ unsigned red[4];
    const int tid = threadIdx.x;
    const int64_t clip = blockIdx.y;
    const float* __restrict__ pp = peak_partials + clip * n_partials;
    unsigned peak = 0u;
    for (int64_t i = tid; i < n_partials; i += 256) peak = rs_umax(peak, rs_absbits(pp[i]));
    peak = rs_wave_umax(peak);
    if ((tid & 63) == 0) red[tid >> 6] = peak;
    __syncthreads();
    peak = rs_umax(rs_umax(red[0], red[1]), rs_umax(red[2], red[3]));
    if (peak == 0u) return;
    const float d = __uint_as_float(peak);
    float* __restrict__ yc = y + clip * Lout;
    const int64_t n0 = (int64_t)blockIdx.x * RS_NORM_CHUNK;
    const int64_t n1 = n0 + RS_NORM_CHUNK < Lout ? n0 + RS_NORM_CHUNK : Lout;
    for (int64_t n = n0 + tid; n < n1; n += 256) yc[n] = yc[n] / d;
}

inline bool rs_direct(int orig, int nnew) { return nnew <= RS_DIRECT_MAX_NEW && orig <= RS_DIRECT_MAX_ORIG; }
inline bool rs_ratio_ok(int orig, int nnew, int width) {
    return orig >= 1 && nnew >= 1 && width >= 0 && nnew <= RS_MAX_PHASES && orig <= RS_MAX_TAPS && width <= RS_MAX_TAPS &&
           2 * width + orig <= RS_MAX_TAPS;
}
inline int64_t rs_out_len(int64_t L, int orig, int nnew) { return (L * nnew + orig - 1) / orig; }
inline int64_t rs_workgroups(int64_t Lout, int orig, int nnew) {
    const int64_t frames = (Lout + nnew - 1) / nnew, tile = rs_direct(orig, nnew) ? RS_DIRECT_TILE : RS_TILE;
    return (frames + tile - 1) / tile;
}

}  // namespace

extern "C" int tt_resample_tile(void) { return RS_TILE; }
extern "C" int tt_resample_direct_tile(void) { return RS_DIRECT_TILE; }
extern "C" int tt_resample_max_taps(void) { return RS_MAX_TAPS; }
extern "C" int tt_resample_max_phases(void) { return RS_MAX_PHASES; }

extern "C" int64_t tt_resample_partials(int64_t L, int orig, int nnew) {
    if (L < 1 || L > (int64_t)1 << 40 || !rs_ratio_ok(orig, nnew, 0)) return TT_E_BADARG;
    return rs_workgroups(rs_out_len(L, orig, nnew), orig, nnew);
}

extern "C" int tt_resample(const float* x, int B, int C, int64_t L, const float* taps_t, int orig, int nnew, int width, float* y,
                           int64_t Lout, float* peak_partials, void* stream) {
    if (!x || !taps_t || !y || B < 1 || C < 1 || L < 1 || L > (int64_t)1 << 40 || !rs_ratio_ok(orig, nnew, width)) return TT_E_BADARG;
    if (Lout != rs_out_len(L, orig, nnew)) return TT_E_BADARG;
    const int64_t nwg = rs_workgroups(Lout, orig, nnew);
    if (nwg > 0x7fffffff || B > 65535) return TT_E_UNSUPPORTED;
    const dim3 grid((unsigned)nwg, B);
    if (rs_direct(orig, nnew)) {
        const size_t lds = (size_t)(RS_DIRECT_TILE * orig + 2 * width) * sizeof(float);
#define RS_LAUNCH_DIRECT(N)                                                                                                            \
    hipLaunchKernelGGL(k_resample_direct<N>, grid, dim3(256), lds, tt_stream(stream), x, C, L, taps_t, orig, width, y, Lout, peak_partials)
        if (nnew == 1) RS_LAUNCH_DIRECT(1);
        else if (nnew == 2) RS_LAUNCH_DIRECT(2);
        else if (nnew == 3) RS_LAUNCH_DIRECT(3);
        else RS_LAUNCH_DIRECT(4);
#undef RS_LAUNCH_DIRECT
    } else {
        const size_t lds = (size_t)(RS_TILE * orig + 2 * width) * sizeof(float);
        hipLaunchKernelGGL(k_resample, grid, dim3(256), lds, tt_stream(stream), x, C, L, taps_t, orig, nnew, width, y, Lout, peak_partials);
    }
    TT_LAUNCH_CHECK();
    return 0;
}

extern "C" int tt_resample_normalize(float* y, int B, int64_t Lout, const float* peak_partials, int64_t n_partials_per_clip, void* stream) {
    if (!y || !peak_partials || B < 1 || Lout < 1 || n_partials_per_clip < 1) return TT_E_BADARG;
    const int64_t nwg = (Lout + RS_NORM_CHUNK - 1) / RS_NORM_CHUNK;
    if (nwg > 0x7fffffff || B > 65535) return TT_E_UNSUPPORTED;
    hipLaunchKernelGGL(k_resample_normalize, dim3((unsigned)nwg, B), dim3(256), 0, tt_stream(stream), y, Lout, peak_partials,
                       n_partials_per_clip);
    TT_LAUNCH_CHECK();
    return 0;
}
