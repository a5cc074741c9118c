// The FiLM layer of TimbreTrapFiLM (reference modules.py:780-889): a per-channel affine map of the latents x (B, D, T), switched by a
// two-entry condition c_r = (transcribe, not transcribe):
//     G_r[d]  = (gamma.weight[d][0] c_r0 + gamma.weight[d][1] c_r1) + gamma.bias[d]        Bt_r[d] likewise from beta
//     y[r B + b][d][t] = x[b][d][t] G_r[d] + Bt_r[d]                                       r < R: R = 2 is the pair decode (one read of x)
//   k_film_fwd     the map; every product and every sum is rounded on its own, as torch's `x * gamma(c) + beta(c)` rounds them
//   k_film_bwd     dx = sum_r G_r dy_r and, per workgroup, the sums of x dy_r and of dy_r over its frames -> one slot of the workspace each
//   k_film_reduce  per channel: the slots added in float64 in a fixed order, then the four parameter gradients (+=)
// A workgroup covers FILM_TILE frames of one (clip, channel) row, a thread four consecutive ones: as one 16-byte access where the rows
// allow it, as four scalar ones otherwise -- the same values through the same additions either way.  No atomics; element offsets are 64-bit.
#include "common.h"

// the reference rounds x * G and (x * G) + Bt separately, and so does autograd's sum of the two branches' gradients: nothing in this file
// may be contracted into a fused multiply-add
#pragma clang fp contract(off)

namespace {

constexpr int FILM_TILE = 1024;          // frames per workgroup: 256 threads x 4

struct FilmCond { float c[4]; };         // c[2 r + j], read from host memory at launch

__device__ __forceinline__ float film_coef(const float* __restrict__ w, const float* __restrict__ b, int d, float c0, float c1) {
    const float p0 = w[2 * (long)d] * c0, p1 = w[2 * (long)d + 1] * c1;
    return (p0 + p1) + b[d];
}

template <bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ p, long t, long T, float (&v)[4]) {
    if (VEC) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = t + k < T ? p[k] : 0.f;
    }
}

template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ p, long t, long T, const float (&v)[4]) {
    if (VEC) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (t + k < T) p[k] = v[k];
    }
}

// items = B D tiles work items (clip, channel, tile of frames), walked with a grid stride; half = B D T, the elements of one condition's output
template <bool VEC, int R>
__global__ __launch_bounds__(256) void k_film_fwd(const float* __restrict__ x, const float* __restrict__ gw, const float* __restrict__ gb,
                                                  const float* __restrict__ bw, const float* __restrict__ bb, FilmCond cond,
                                                  float* __restrict__ y, long items, long tiles, int D, long T, long half) {
    for (long item = blockIdx.x; item < items; item += gridDim.x) {
        const long row = item / tiles, tile = item - row * tiles;
        const int d = (int)(row % D);
        const long t = tile * FILM_TILE + 4 * (long)threadIdx.x;
        if (t >= T) continue;
        const long o = row * T + t;
        float v[4];
        load4<VEC>(x + o, t, T, v);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float G = film_coef(gw, gb, d, cond.c[2 * r], cond.c[2 * r + 1]);
            const float Bt = film_coef(bw, bb, d, cond.c[2 * r], cond.c[2 * r + 1]);
            float out[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float p = v[k] * G;
                out[k] = p + Bt;
            }
            store4<VEC>(y + r * half + o, t, T, out);
        }
    }
}

// part (NULL: no parameter gradients, x is not read): [R][2][D][n] floats, n = B tiles slots per channel; slot b tiles + tile of
// [r][0] holds this workgroup's sum of x dy_r, of [r][1] its sum of dy_r.  A thread adds its (at most four) terms in frame order, the
// workgroup combines its threads pairwise (the lanes of a wavefront by butterfly, the four wavefronts as (0 + 1) + (2 + 3)).
template <bool VEC, int R>
__global__ __launch_bounds__(256) void k_film_bwd(const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ gw,
                                                  const float* __restrict__ gb, FilmCond cond, float* __restrict__ dx,
                                                  float* __restrict__ part, long items, long tiles, int D, long T, long half, long n) {
    __shared__ float red[4][2 * R];
    for (long item = blockIdx.x; item < items; item += gridDim.x) {
        const long row = item / tiles, tile = item - row * tiles;
        const int d = (int)(row % D);
        const long b = row / D;
        const long t = tile * FILM_TILE + 4 * (long)threadIdx.x;
        float acc[2 * R];
#pragma unroll
        for (int q = 0; q < 2 * R; ++q) acc[q] = 0.f;
        if (t < T) {
            const long o = row * T + t;
            float xv[4] = {0.f, 0.f, 0.f, 0.f}, g[4] = {0.f, 0.f, 0.f, 0.f};
            if (part) load4<VEC>(x + o, t, T, xv);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float dv[4];
                load4<VEC>(dy + r * half + o, t, T, dv);
                const float G = film_coef(gw, gb, d, cond.c[2 * r], cond.c[2 * r + 1]);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float p = G * dv[k];
                    g[k] = r == 0 ? p : g[k] + p;
                    if (VEC || t + k < T) {
                        acc[2 * r] += xv[k] * dv[k];
                        acc[2 * r + 1] += dv[k];
                    }
                }
            }
            if (dx) store4<VEC>(dx + o, t, T, g);
        }
        if (part) {
#pragma unroll
            for (int q = 0; q < 2 * R; ++q) {
                const float s = wave_sum(acc[q]);
                if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = s;
            }
            __syncthreads();
            if (threadIdx.x < 2 * R) {
                const int q = threadIdx.x;
                part[((long)q * D + d) * n + b * tiles + tile] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
            }
            __syncthreads();
        }
    }
}

// one wavefront per channel: lane l adds slots l, l + 64, ... in float64, the lanes combine by butterfly, lane 0 forms the gradients
template <int R>
__global__ __launch_bounds__(64) void k_film_reduce(const float* __restrict__ part, FilmCond cond, float* __restrict__ dgw,
                                                    float* __restrict__ dgb, float* __restrict__ dbw, float* __restrict__ dbb, int D, long n) {
    const long d = blockIdx.x;
    double s[2 * R];
#pragma unroll
    for (int q = 0; q < 2 * R; ++q) {
        const float* src = part + ((long)q * D + d) * n;
        double a = 0.0;
        for (long i = threadIdx.x; i < n; i += 64) a += (double)src[i];
        s[q] = wave_sum_d(a);
    }
    if (threadIdx.x != 0) return;
    double w0 = 0.0, w1 = 0.0, wb = 0.0, v0 = 0.0, v1 = 0.0, vb = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const double c0 = (double)cond.c[2 * r], c1 = (double)cond.c[2 * r + 1], P = s[2 * r], S = s[2 * r + 1];
        w0 += c0 * P; w1 += c1 * P; wb += P;
        v0 += c0 * S; v1 += c1 * S; vb += S;
    }
    dgw[2 * d] += (float)w0; dgw[2 * d + 1] += (float)w1; dgb[d] += (float)wb;
    dbw[2 * d] += (float)v0; dbw[2 * d + 1] += (float)v1; dbb[d] += (float)vb;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline long film_tiles(int T) { return ((long)T + FILM_TILE - 1) / FILM_TILE; }
inline unsigned film_grid(long items) {
    const long cap = 8L * tt_cus();
    return (unsigned)(items < cap ? items : cap);
}
inline FilmCond film_cond(const float* cond, int R) {
    FilmCond c = {{0.f, 0.f, 0.f, 0.f}};
    for (int i = 0; i < 2 * R; ++i) c.c[i] = cond[i];
    return c;
}

}  // namespace

extern "C" int tt_film_tile_frames(void) { return FILM_TILE; }

extern "C" int64_t tt_film_scratch_bytes(int B, int D, int T, int R) {
    if (B <= 0 || D <= 0 || T <= 0 || R < 1 || R > 2) return 0;
    return (int64_t)R * 2 * D * B * film_tiles(T) * 4;
}

extern "C" int tt_film_fwd(const float* x, const float* gw, const float* gb, const float* bw, const float* bb, const float* cond, float* y,
                           int B, int D, int T, int R, void* stream) {
    if (!x || !gw || !gb || !bw || !bb || !cond || !y || B <= 0 || D <= 0 || T <= 0 || R < 1 || R > 2) return TT_E_BADARG;
    const long tiles = film_tiles(T), items = (long)B * D * tiles, half = (long)B * D * T;
    const FilmCond c = film_cond(cond, R);
    const bool vec = T % 4 == 0 && aligned16(x) && aligned16(y);
    const dim3 grid(film_grid(items)), block(256);
    hipStream_t st = tt_stream(stream);
#define FILM_FWD(V, RR) hipLaunchKernelGGL((k_film_fwd<V, RR>), grid, block, 0, st, x, gw, gb, bw, bb, c, y, items, tiles, D, (long)T, half)
    if (vec) { if (R == 2) FILM_FWD(true, 2); else FILM_FWD(true, 1); }
    else     { if (R == 2) FILM_FWD(false, 2); else FILM_FWD(false, 1); }
#undef FILM_FWD
    TT_LAUNCH_CHECK();
    return 0;
}

extern "C" int tt_film_bwd(const float* x, const float* dy, const float* gw, const float* gb, const float* cond, float* dx, float* dgw,
                           float* dgb, float* dbw, float* dbb, void* ws, int B, int D, int T, int R, void* stream) {
    const int grads = (dgw != nullptr) + (dgb != nullptr) + (dbw != nullptr) + (dbb != nullptr);
    if (!dy || !gw || !gb || !cond || B <= 0 || D <= 0 || T <= 0 || R < 1 || R > 2) return TT_E_BADARG;
    if ((grads != 0 && grads != 4) || (grads && (!x || !ws))) return TT_E_BADARG;
    if (!dx && !grads) return 0;
    const long tiles = film_tiles(T), items = (long)B * D * tiles, half = (long)B * D * T, n = (long)B * tiles;
    const FilmCond c = film_cond(cond, R);
    const bool vec = T % 4 == 0 && aligned16(dy) && (!dx || aligned16(dx)) && (!grads || aligned16(x));
    float* part = grads ? (float*)ws : nullptr;
    const dim3 grid(film_grid(items)), block(256);
    hipStream_t st = tt_stream(stream);
#define FILM_BWD(V, RR) hipLaunchKernelGGL((k_film_bwd<V, RR>), grid, block, 0, st, x, dy, gw, gb, c, dx, part, items, tiles, D, (long)T, half, n)
    if (vec) { if (R == 2) FILM_BWD(true, 2); else FILM_BWD(true, 1); }
    else     { if (R == 2) FILM_BWD(false, 2); else FILM_BWD(false, 1); }
#undef FILM_BWD
    TT_LAUNCH_CHECK();
    if (grads) {
        if (R == 2) hipLaunchKernelGGL((k_film_reduce<2>), dim3((unsigned)D), dim3(64), 0, st, (const float*)part, c, dgw, dgb, dbw, dbb, D, n);
        else        hipLaunchKernelGGL((k_film_reduce<1>), dim3((unsigned)D), dim3(64), 0, st, (const float*)part, c, dgw, dgb, dbw, dbb, D, n);
        TT_LAUNCH_CHECK();
    }
    return 0;
}
