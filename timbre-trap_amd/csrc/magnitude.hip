// Front end of the magnitude variants (reference modules.py:892-1075, cqtwrapper.py:122-182):
//   k_magnitude   CQT.to_magnitude: (..., 2, F, T) re / im planes -> (..., F, T) |c|
//   k_db_max      CQT.to_decibels, step 1: per item of dim 0, the largest 20 log10(max(m, 1e-10)) of a slice -> one partial per workgroup
//   k_db_map      step 2: every workgroup first reduces its item's DB_PARTS partials (a fixed order: bit-identical from run to run), then
//                 d = max(20 log10(max(m, 1e-10)), top - 80), optionally 1 + (d - top) / 80
// The dB step restates torchaudio AmplitudeToDB('amplitude', top_db=80) item by item, as the reference loop does; both are streaming
// kernels (one read and one write of the tensor, plus one read for the maximum).
#include "common.h"

namespace {

constexpr int DB_PARTS = 64;             // workgroups per item of the maximum pass; k_db_map reads them with one wave

__global__ __launch_bounds__(256) void k_magnitude(const float* __restrict__ x, float* __restrict__ y, long outer, long inner) {
    const long total = outer * inner;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long o = i / inner, r = i - o * inner;
        const float re = x[(2 * o) * inner + r], im = x[(2 * o + 1) * inner + r];
        y[i] = sqrtf(re * re + im * im);
    }
}

// NaN propagates as in torch's clamp / max / maximum (fmaxf alone would drop it): a clip holding a NaN comes out all NaN, as on the
// reference path, instead of finite
__device__ __forceinline__ float nanmax(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : fmaxf(a, b); }
__device__ __forceinline__ float to_db(float m) { return 20.f * log10f(m != m ? m : fmaxf(m, 1e-10f)); }

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = nanmax(v, __shfl_xor(v, o, 64));
    return v;
}

// grid (DB_PARTS, items)
__global__ __launch_bounds__(256) void k_db_max(const float* __restrict__ m, float* __restrict__ part, long per_item) {
    __shared__ float red[4];
    const float* src = m + (long)blockIdx.y * per_item;
    float mx = -INFINITY;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per_item; i += (long)DB_PARTS * 256) mx = nanmax(mx, to_db(src[i]));
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) part[(long)blockIdx.y * DB_PARTS + blockIdx.x] = nanmax(nanmax(red[0], red[1]), nanmax(red[2], red[3]));
}

// grid (chunks, items)
__global__ __launch_bounds__(256) void k_db_map(const float* __restrict__ m, float* __restrict__ out, const float* __restrict__ part,
                                                long per_item, int rescale) {
    __shared__ float top_s;
    if (threadIdx.x < 64) {
        const float v = wave_max(part[(long)blockIdx.y * DB_PARTS + threadIdx.x]);
        if (threadIdx.x == 0) top_s = v;
    }
    __syncthreads();
    const float top = top_s, floor_db = top - 80.f;
    const float* src = m + (long)blockIdx.y * per_item;
    float* dst = out + (long)blockIdx.y * per_item;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per_item; i += (long)gridDim.x * 256) {
        float d = nanmax(to_db(src[i]), floor_db);
        if (rescale) d = 1.f + (d - top) / 80.f;
        dst[i] = d;
    }
}

inline int grid_1d(long n, int cap) {
    long g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

}  // namespace

extern "C" int tt_magnitude(const float* x, float* y, int64_t outer, int64_t inner, void* stream) {
    if (!x || !y || outer <= 0 || inner <= 0) return TT_E_BADARG;
    hipLaunchKernelGGL(k_magnitude, dim3(grid_1d(outer * inner, 16 * tt_cus())), dim3(256), 0, tt_stream(stream), x, y, (long)outer, (long)inner);
    TT_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t tt_decibels_scratch_bytes(int64_t items) { return items > 0 ? items * DB_PARTS * 4 : 0; }

extern "C" int tt_decibels(const float* m, float* out, int64_t items, int64_t per_item, int rescale, float* ws, void* stream) {
    if (!m || !out || !ws || items <= 0 || items > 65535 || per_item <= 0) return TT_E_BADARG;
    hipStream_t st = tt_stream(stream);
    hipLaunchKernelGGL(k_db_max, dim3(DB_PARTS, (unsigned)items), dim3(256), 0, st, m, ws, (long)per_item);
    TT_LAUNCH_CHECK();
    long chunks = (per_item + 256 * 8 - 1) / (256 * 8);
    const long cap = (16L * tt_cus() + items - 1) / items;
    if (chunks > cap) chunks = cap;
    if (chunks < 1) chunks = 1;
    hipLaunchKernelGGL(k_db_map, dim3((unsigned)chunks, (unsigned)items), dim3(256), 0, st, m, out, (const float*)ws, (long)per_item,
                       rescale ? 1 : 0);
    TT_LAUNCH_CHECK();
    return 0;
}
