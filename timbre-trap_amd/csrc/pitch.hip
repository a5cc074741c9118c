// Frame-level pitch annotations to batched targets on the device (include/ttrap.h: tt_pitch_*): float64 comparisons, integers and the
// float64 blur of losses.hip's k_tgt_blur; no atomics, no F x T work buffer, a launch count that does not depend on the batch.
//
//   arena (uploaded once per dataset): times float64, trk int64 [n_tracks][4] = {base, K, below, above}, row_off int64, bins int32 per
//   value (-1: dropped), lost uint8 per row -- track n's source frame i is arena row trk[n].base + i.
//
//   track[B], target times (B, T) --k_pitch_nearest--> idx (B, T)             (the source frame each item's frame reads)
//   idx, arena --k_pitch_min--> part[b][tile], lost[b][tile]                  (smallest blurred value over the tile's painted positions)
//              --k_pitch_reduce--> minv[b], flags[b]                          (a minimum and an OR: neither depends on the order)
//   idx, arena, minv --k_pitch_write--> out (B, F, T) float64 or float32      (every element written once)
//
// k_pitch_min / k_pitch_write: one workgroup per tile of PITCH_TILE frames of one item, lane = frame.  The painted bins of a frame are a
// bitmask in LDS, word w of frame t at s_mask[w * PITCH_TILE + t] -- a lane only ever touches its own column, so the bank is the lane
// and nothing conflicts.  The lane that owns a frame ORs its source row's bins into the column (a duplicate bin paints once, as the
// reference's fancy-index assignment does).  A blurred value is formed from the 2 r + 1 mask bits around (bin, t) in SciPy's order
// (centre, then the pairs from the outside in, separate multiply and add); with a in {0, 1} a pair that holds no one contributes
// (0 + 0) w = +0 and acc + (+0) = acc exactly, so such pairs are skipped, and a window without a one is +0 outright.
// k_pitch_write walks the mask 32 bins at a time: the three words around the current one stay in registers and every window is two
// shifts; the four waves of a workgroup take the words round-robin and each store is 64 consecutive elements of one row.
#include "common.h"

#define PITCH_TILE 64                           // = tt_pitch_tile_frames(): frames per workgroup (one lane each)
#define PITCH_MAX_BINS 1024                     // = tt_pitch_max_bins(): mask bits per frame held in LDS
#define PITCH_WORDS (PITCH_MAX_BINS / 32)
#define PITCH_MAX_RADIUS 31                     // = tt_pitch_max_radius(): a window of 2 r + 1 <= 63 bits fits one 64-bit register
#define PITCH_EMPTY 1.0e300                     // k_tgt_seed_min's identity: no painted position

static_assert(PITCH_TILE == 64, "one wavefront of lanes paints a tile");

namespace {

__global__ __launch_bounds__(256) void k_pitch_nearest(const double* __restrict__ times, const long* __restrict__ trk, int n_tracks,
                                                       const int* __restrict__ track, const double* __restrict__ target, int B, int T,
                                                       int* __restrict__ idx) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * T) return;
    const int tr = track[i / T];
    if (tr < 0 || tr >= n_tracks) {             // no such track: an empty frame for the target kernels
        idx[i] = -1;
        return;
    }
    const long K = trk[4 * (long)tr + 1];
    if (K < 1) {
        idx[i] = -1;
        return;
    }
    const double* __restrict__ src = times + trk[4 * (long)tr];
    const double x = target[i];
    // number of midpoints src[m] / 2 + src[m + 1] / 2 (K - 1 of them, non-decreasing) that are < x; a NaN sorts after all of them
    long l = 0, h = K - 1;
    if (x != x) l = h;
    while (l < h) {
        const long m = l + ((h - l) >> 1);
        const double mid = __dadd_rn(__dmul_rn(src[m], 0.5), __dmul_rn(src[m + 1], 0.5));
        if (mid < x) l = m + 1;
        else h = m;
    }
    if (x < src[0]) l = trk[4 * (long)tr + 2];
    if (x > src[K - 1]) l = trk[4 * (long)tr + 3];
    idx[i] = (int)l;
}

// the arena row frame (b, t) reads, or -1
__device__ __forceinline__ long pitch_row(const long* __restrict__ trk, int n_tracks, int tr, int i) {
    if (tr < 0 || tr >= n_tracks || i < 0 || (long)i >= trk[4 * (long)tr + 1]) return -1;
    return trk[4 * (long)tr] + i;
}

// zero the tile's mask, then every frame's lane paints its row; returns the row of the calling lane's frame (-1: none, or not a painter)
__device__ __forceinline__ long pitch_paint(unsigned* s_mask, const long* __restrict__ trk, int n_tracks, const int* __restrict__ track,
                                            const int* __restrict__ idx, const long* __restrict__ row_off,
                                            const int* __restrict__ bins, int F, int T, int b, int t0) {
    for (int k = threadIdx.x; k < PITCH_WORDS * PITCH_TILE; k += blockDim.x) s_mask[k] = 0u;
    __syncthreads();
    long row = -1;
    const int t = t0 + threadIdx.x;
    if (threadIdx.x < PITCH_TILE && t < T) {
        row = pitch_row(trk, n_tracks, track[b], idx[(long)b * T + t]);
        if (row >= 0) {
            for (long v = row_off[row]; v < row_off[row + 1]; ++v) {
                const int f = bins[v];
                if (f >= 0 && f < F) s_mask[(f >> 5) * PITCH_TILE + threadIdx.x] |= 1u << (f & 31);
            }
        }
    }
    __syncthreads();
    return row;
}

// bit k of the result = mask bit (32 (wi - 1) + o + k) of the words prev (wi - 1), cur (wi), next (wi + 1), 1 <= o <= 63, cut to `keep`
__device__ __forceinline__ unsigned long long pitch_window(unsigned prev, unsigned cur, unsigned next, int o, unsigned long long keep) {
    const unsigned long long lo = (unsigned long long)prev | ((unsigned long long)cur << 32);
    return ((lo >> o) | ((unsigned long long)next << (64 - o))) & keep;
}

// k_tgt_blur's value at the centre of window u (bit r = the position itself) for a map of zeros and ones
__device__ __forceinline__ double pitch_blur(unsigned long long u, const double* s_w, int r) {
    double acc = __dmul_rn((double)((u >> r) & 1ull), s_w[r]);
    for (int j = -r; j < 0; ++j) {
        const int pair = (int)((u >> (r + j)) & 1ull) + (int)((u >> (r - j)) & 1ull);
        if (pair) acc = __dadd_rn(acc, __dmul_rn((double)pair, s_w[r + j]));
    }
    return acc;
}

__device__ __forceinline__ unsigned pitch_word(const unsigned* s_mask, int w, int lane) {
    return (w >= 0 && w < PITCH_WORDS) ? s_mask[w * PITCH_TILE + lane] : 0u;
}

__global__ __launch_bounds__(PITCH_TILE) void k_pitch_min(const long* __restrict__ trk, int n_tracks, const int* __restrict__ track,
                                                          const int* __restrict__ idx, const long* __restrict__ row_off,
                                                          const int* __restrict__ bins, const unsigned char* __restrict__ lost,
                                                          const double* __restrict__ w, int r, int F, int T, double* __restrict__ part,
                                                          int* __restrict__ part_lost) {
    __shared__ unsigned s_mask[PITCH_WORDS * PITCH_TILE];
    __shared__ double s_w[2 * PITCH_MAX_RADIUS + 1];
    __shared__ double s_red[PITCH_TILE];
    const int lane = threadIdx.x, b = blockIdx.y;
    for (int k = lane; r > 0 && k < 2 * r + 1; k += PITCH_TILE) s_w[k] = w[k];          // radius 0: no weights, w may be NULL
    const long row = pitch_paint(s_mask, trk, n_tracks, track, idx, row_off, bins, F, T, b, blockIdx.x * PITCH_TILE);
    double m = PITCH_EMPTY;
    int any_lost = 0;
    if (row >= 0) {
        any_lost = lost[row] != 0;
        if (r > 0) {
            const unsigned long long keep = (1ull << (2 * r + 1)) - 1ull;
            for (long v = row_off[row]; v < row_off[row + 1]; ++v) {
                const int f = bins[v];
                if (f < 0 || f >= F) continue;
                const int wi = f >> 5;
                const unsigned long long u = pitch_window(pitch_word(s_mask, wi - 1, lane), pitch_word(s_mask, wi, lane),
                                                          pitch_word(s_mask, wi + 1, lane), 32 + (f & 31) - r, keep);
                m = fmin(m, pitch_blur(u, s_w, r));
            }
        }
    }
    const unsigned long long lost_lanes = __ballot(any_lost);
    s_red[lane] = m;
    __syncthreads();
    for (int s = PITCH_TILE / 2; s > 0; s >>= 1) {
        if (lane < s) s_red[lane] = fmin(s_red[lane], s_red[lane + s]);
        __syncthreads();
    }
    if (lane == 0) {
        const long p = (long)b * gridDim.x + blockIdx.x;
        part[p] = s_red[0];
        part_lost[p] = lost_lanes != 0ull;
    }
}

// minv[b] = smallest of item b's `tiles` partials, flags[b] = OR of its lost words: one workgroup per item
__global__ __launch_bounds__(64) void k_pitch_reduce(const double* __restrict__ part, const int* __restrict__ part_lost, int tiles,
                                                     double* __restrict__ minv, int* __restrict__ flags) {
    __shared__ double s_red[64];
    const int lane = threadIdx.x, b = blockIdx.x;
    double m = PITCH_EMPTY;
    int any_lost = 0;
    for (long k = lane; k < tiles; k += 64) {
        m = fmin(m, part[(long)b * tiles + k]);
        any_lost |= part_lost[(long)b * tiles + k];
    }
    const unsigned long long lost_lanes = __ballot(any_lost);
    s_red[lane] = m;
    __syncthreads();
    for (int s = 32; s > 0; s >>= 1) {
        if (lane < s) s_red[lane] = fmin(s_red[lane], s_red[lane + s]);
        __syncthreads();
    }
    if (lane == 0) {
        minv[b] = s_red[0];
        flags[b] = lost_lanes != 0ull;
    }
}

template <typename OUT>
__global__ __launch_bounds__(256) void k_pitch_write(const long* __restrict__ trk, int n_tracks, const int* __restrict__ track,
                                                     const int* __restrict__ idx, const long* __restrict__ row_off,
                                                     const int* __restrict__ bins, const double* __restrict__ w, int r, int F, int T,
                                                     const double* __restrict__ minv, OUT* __restrict__ out) {
    __shared__ unsigned s_mask[PITCH_WORDS * PITCH_TILE];
    __shared__ double s_w[2 * PITCH_MAX_RADIUS + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y;
    const int t0 = blockIdx.x * PITCH_TILE;
    for (int k = threadIdx.x; r > 0 && k < 2 * r + 1; k += 256) s_w[k] = w[k];
    pitch_paint(s_mask, trk, n_tracks, track, idx, row_off, bins, F, T, b, t0);
    const int t = t0 + lane;
    if (t >= T) return;
    const double mn = r > 0 ? minv[b] : 1.0;
    const unsigned long long keep = (1ull << (2 * r + 1)) - 1ull;
    OUT* __restrict__ col = out + (long)b * F * T + t;
    for (int wi = wave; wi * 32 < F; wi += 4) {
        const unsigned prev = pitch_word(s_mask, wi - 1, lane), cur = pitch_word(s_mask, wi, lane), next = pitch_word(s_mask, wi + 1, lane);
        const bool blank = (prev | cur | next) == 0u;
        const int f1 = F - wi * 32 < 32 ? F - wi * 32 : 32;
        for (int k = 0; k < f1; ++k) {
            double v = 0.0;
            if (!blank) {
                if (r == 0) v = (double)((cur >> k) & 1u);
                else {
                    const unsigned long long u = pitch_window(prev, cur, next, 32 + k - r, keep);
                    if (u) {
                        v = pitch_blur(u, s_w, r) / mn;
                        v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
                    }
                }
            }
            col[(long)(wi * 32 + k) * T] = (OUT)v;
        }
    }
}

}  // namespace

extern "C" int tt_pitch_tile_frames(void) { return PITCH_TILE; }
extern "C" int tt_pitch_max_bins(void) { return PITCH_MAX_BINS; }
extern "C" int tt_pitch_max_radius(void) { return PITCH_MAX_RADIUS; }

static inline long pitch_tiles(int T) { return ((long)T + PITCH_TILE - 1) / PITCH_TILE; }

extern "C" int64_t tt_pitch_scratch_bytes(int B, int T) {
    if (B < 1 || T < 1) return 0;
    return (int64_t)B * (pitch_tiles(T) + 1) * (int64_t)(sizeof(double) + sizeof(int));
}

extern "C" int tt_pitch_nearest(const double* times, const int64_t* tracks, int n_tracks, const int* track, const double* target, int B,
                                int T, int* idx, void* stream) {
    if (B < 0 || T < 0 || n_tracks < 0 || (n_tracks > 0 && (!times || !tracks))) return TT_E_BADARG;
    const long n = (long)B * T;
    if (n == 0) return 0;
    if (!track || !target || !idx || (n + 255) / 256 > 0x7fffffffL) return TT_E_BADARG;
    hipLaunchKernelGGL(k_pitch_nearest, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, tt_stream(stream), times,
                       reinterpret_cast<const long*>(tracks), n_tracks, track, target, B, T, idx);
    TT_LAUNCH_CHECK();
    return 0;
}

extern "C" int tt_pitch_targets(const int* idx, const int64_t* tracks, int n_tracks, const int* track, int B, int T, const int64_t* row_off,
                                const int* bins, const unsigned char* lost, const double* weights, int radius, int F, int out_float32,
                                void* scratch, void* out, int* flags, void* stream) {
    if (B < 0 || T < 0 || n_tracks < 0 || F < 1 || F > PITCH_MAX_BINS || radius < 0 || radius > PITCH_MAX_RADIUS || B > 65535)
        return TT_E_BADARG;
    if (B == 0 || T == 0) return 0;
    if (!idx || !track || !out || !flags || !scratch || (radius > 0 && !weights) || (n_tracks > 0 && (!tracks || !row_off || !lost)))
        return TT_E_BADARG;
    hipStream_t st = tt_stream(stream);
    const long tiles = pitch_tiles(T);
    // scratch: part[B][tiles], minv[B] (float64), then part_lost[B][tiles] (int)
    double* part = static_cast<double*>(scratch);
    double* minv = part + (long)B * tiles;
    int* part_lost = reinterpret_cast<int*>(minv + B);
    const long* trk = reinterpret_cast<const long*>(tracks);
    const long* off = reinterpret_cast<const long*>(row_off);
    const dim3 grid((unsigned)tiles, (unsigned)B);
    hipLaunchKernelGGL(k_pitch_min, grid, dim3(PITCH_TILE), 0, st, trk, n_tracks, track, idx, off, bins, lost, weights, radius, F, T, part,
                       part_lost);
    TT_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_pitch_reduce, dim3(B), dim3(64), 0, st, (const double*)part, (const int*)part_lost, (int)tiles, minv, flags);
    TT_LAUNCH_CHECK();
    if (out_float32)
        hipLaunchKernelGGL(k_pitch_write<float>, grid, dim3(256), 0, st, trk, n_tracks, track, idx, off, bins, weights, radius, F, T,
                           (const double*)minv, static_cast<float*>(out));
    else
        hipLaunchKernelGGL(k_pitch_write<double>, grid, dim3(256), 0, st, trk, n_tracks, track, idx, off, bins, weights, radius, F, T,
                           (const double*)minv, static_cast<double*>(out));
    TT_LAUNCH_CHECK();
    return 0;
}
