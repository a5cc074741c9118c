// Random stem mixtures for training batches on the device (include/ttrap.h: tt_mix_*): the excerpt gather-and-sum of the audio and the
// segmented sum-and-clamp of the stems' target maps.  No atomics, no scratch, no LDS: every output element is formed by one lane from
// a chain of additions in stem order, so a result does not depend on the launch geometry and is identical from run to run.
//
//   arena (uploaded once per dataset): every track's samples fp32, concatenated; tracks int64 [n_tracks][2] = {base, length}
//   stem s of item b (item_off[b] <= s < item_off[b + 1]) reads track stem_track[s] from sample stem_start[s] on; a negative start is
//   silence in front of the track, whatever lies beyond the track's end is silence too
//
// Both kernels: one workgroup per MIX_TILE consecutive elements of one output row, a lane owns four consecutive elements ("quad").
// The quads are laid on the OUTPUT's 16-byte grid: row b begins `row` elements into the buffer, so its first quad begins o <= 0
// elements before the row (o = -((row + misalignment of the pointer) mod 4 elements of 16 bytes)) and every quad that lies inside the
// row is one aligned 16-byte store; only the row's first and last quad store element by element.  A stem's source then is 16-byte
// aligned for every lane or for none: the workgroup picks the 16-byte-load path or the dword path once per stem (a uniform branch),
// and only a tile that touches an end of the track, or of the row, takes the path with per-element bounds predicates.
#include "common.h"

#define MIX_TILE 1024                           // = tt_mix_tile() = tt_mix_targets_tile(): output elements per workgroup
#define MIX_THREADS (MIX_TILE / 4)

namespace {

// one 16-byte memory operation each: native vectors, so that the compiler keeps the aligned path apart from the element-wise one
typedef float mix_f4 __attribute__((ext_vector_type(4)));
typedef double mix_d2 __attribute__((ext_vector_type(2)));

// elements in front of the row's first sample at which its first quad begins (0 .. 3), for an element of `esz` bytes whose row begins
// `row` elements behind `p`; `quantum` = elements per aligned unit (16 bytes of the element type)
__device__ __host__ __forceinline__ int mix_lead(const void* p, long row, int esz, int quantum) {
    const long at = (long)(((uintptr_t)p / (uintptr_t)esz) % (uintptr_t)quantum) + row % quantum;
    return (int)(at % quantum);
}

__device__ __host__ __forceinline__ long mix_tiles(long n, int lead) { return (n + lead + MIX_TILE - 1) / MIX_TILE; }

// the four samples i .. i + 3 of one stem (i may be negative in a row's first quad: such elements are not stored)
__device__ __forceinline__ float4 mix_stem_quad(const float* __restrict__ arena, const long* __restrict__ trk, int n_tracks,
                                                const int* __restrict__ stem_track, const long* __restrict__ stem_start, int s, long i,
                                                long tile_lo, long tile_hi) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    const int tr = stem_track[s];
    if (tr < 0 || tr >= n_tracks) return v;      // the entry's callers check the ids on the host; the kernel still never reads outside the table
    const long base = trk[2 * (long)tr], len = trk[2 * (long)tr + 1], start = stem_start[s];
    const float* __restrict__ src = arena + base + start;
    // uniform over the workgroup: the tile's whole span [tile_lo, tile_hi) lies inside the track
    if (start + tile_lo >= 0 && start + tile_hi <= len) {
        if ((((uintptr_t)(src + tile_lo)) & 15u) == 0) {
            const mix_f4 q = *reinterpret_cast<const mix_f4*>(__builtin_assume_aligned(src + i, 16));
            v = make_float4(q.x, q.y, q.z, q.w);
        } else {
            v.x = src[i];
            v.y = src[i + 1];
            v.z = src[i + 2];
            v.w = src[i + 3];
        }
    } else {
        const long p = start + i;
        if (p >= 0 && p < len) v.x = src[i];
        if (p + 1 >= 0 && p + 1 < len) v.y = src[i + 1];
        if (p + 2 >= 0 && p + 2 < len) v.z = src[i + 2];
        if (p + 3 >= 0 && p + 3 < len) v.w = src[i + 3];
    }
    return v;
}

__device__ __forceinline__ void mix_add(float4& a, const float4& v) {
    a.x += v.x;
    a.y += v.y;
    a.z += v.z;
    a.w += v.w;
}

// the sum of stems s0 .. s1 - 1 in stem order, from +0; two stems' loads are in flight before the first is added
__device__ __forceinline__ float4 mix_group(const float* __restrict__ arena, const long* __restrict__ trk, int n_tracks,
                                            const int* __restrict__ stem_track, const long* __restrict__ stem_start, int s0, int s1, long i,
                                            long tile_lo, long tile_hi) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int s = s0;
    for (; s + 1 < s1; s += 2) {
        const float4 v0 = mix_stem_quad(arena, trk, n_tracks, stem_track, stem_start, s, i, tile_lo, tile_hi);
        const float4 v1 = mix_stem_quad(arena, trk, n_tracks, stem_track, stem_start, s + 1, i, tile_lo, tile_hi);
        mix_add(acc, v0);
        mix_add(acc, v1);
    }
    if (s < s1) mix_add(acc, mix_stem_quad(arena, trk, n_tracks, stem_track, stem_start, s, i, tile_lo, tile_hi));
    return acc;
}

__global__ __launch_bounds__(MIX_THREADS) void k_mix_audio(const float* __restrict__ arena, const long* __restrict__ trk, int n_tracks,
                                                           const int* __restrict__ stem_track, const long* __restrict__ stem_start,
                                                           const int* __restrict__ item_off, const int* __restrict__ item_split, long N,
                                                           long tiles, float* __restrict__ y) {
    const long b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const int lead = mix_lead(y, b * N, 4, 4);
    // the tile's span of the row, and the lane's quad in it
    const long tile_lo = tile * MIX_TILE - lead, tile_hi = tile_lo + MIX_TILE;
    const long i = tile_lo + 4 * (long)threadIdx.x;
    if (i >= N) return;
    const int s0 = item_off[b], s2 = item_off[b + 1];
    int s1 = s0 + item_split[b];
    s1 = s1 < s0 ? s0 : (s1 > s2 ? s2 : s1);
    const float4 a = mix_group(arena, trk, n_tracks, stem_track, stem_start, s0, s1, i, tile_lo, tile_hi);
    const float4 g = mix_group(arena, trk, n_tracks, stem_track, stem_start, s1, s2, i, tile_lo, tile_hi);
    const float4 r = make_float4(a.x + g.x, a.y + g.y, a.z + g.z, a.w + g.w);
    float* __restrict__ out = y + b * N;
    if (i >= 0 && i + 3 < N) {
        *reinterpret_cast<mix_f4*>(__builtin_assume_aligned(out + i, 16)) = mix_f4{r.x, r.y, r.z, r.w};
    } else {
        if (i >= 0) out[i] = r.x;
        if (i + 1 >= 0 && i + 1 < N) out[i + 1] = r.y;
        if (i + 2 >= 0 && i + 2 < N) out[i + 2] = r.z;
        if (i + 3 >= 0 && i + 3 < N) out[i + 3] = r.w;
    }
}

// torch.clamp(v, 0, 1): a NaN fails both comparisons and passes
__device__ __forceinline__ double mix_clamp(double v) { return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v); }

template <typename OUT>
__global__ __launch_bounds__(MIX_THREADS) void k_mix_targets(const double* __restrict__ maps, const int* __restrict__ item_off, long L,
                                                             long tiles, OUT* __restrict__ out) {
    constexpr int Q = 16 / (int)sizeof(OUT);     // elements per 16 bytes of the output
    const long b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const int lead = mix_lead(out, b * L, (int)sizeof(OUT), Q);
    const long tile_lo = tile * MIX_TILE - lead;
    const long i = tile_lo + 4 * (long)threadIdx.x;
    if (i >= L) return;
    const bool whole = i >= 0 && i + 3 < L;     // the lane's quad lies inside the row
    const int s0 = item_off[b], s1 = item_off[b + 1];
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int s = s0; s < s1; ++s) {
        const double* __restrict__ m = maps + (long)s * L;
        if (whole) {
            // uniform over the workgroup's whole quads: this stem's map is 16-byte aligned at every one of them, or at none
            if ((((uintptr_t)(m + tile_lo)) & 15u) == 0) {
                const mix_d2 u = *reinterpret_cast<const mix_d2*>(__builtin_assume_aligned(m + i, 16));
                const mix_d2 w = *reinterpret_cast<const mix_d2*>(__builtin_assume_aligned(m + i + 2, 16));
                a0 += u.x;
                a1 += u.y;
                a2 += w.x;
                a3 += w.y;
            } else {
                const double v0 = m[i], v1 = m[i + 1], v2 = m[i + 2], v3 = m[i + 3];
                a0 += v0;
                a1 += v1;
                a2 += v2;
                a3 += v3;
            }
        } else {
            if (i >= 0) a0 += m[i];
            if (i + 1 >= 0 && i + 1 < L) a1 += m[i + 1];
            if (i + 2 >= 0 && i + 2 < L) a2 += m[i + 2];
            if (i + 3 >= 0 && i + 3 < L) a3 += m[i + 3];
        }
    }
    a0 = mix_clamp(a0);
    a1 = mix_clamp(a1);
    a2 = mix_clamp(a2);
    a3 = mix_clamp(a3);
    OUT* __restrict__ row = out + b * L;
    if (whole) {
        if constexpr (sizeof(OUT) == 4) {
            *reinterpret_cast<mix_f4*>(__builtin_assume_aligned(row + i, 16)) = mix_f4{(float)a0, (float)a1, (float)a2, (float)a3};
        } else {
            *reinterpret_cast<mix_d2*>(__builtin_assume_aligned(row + i, 16)) = mix_d2{a0, a1};
            *reinterpret_cast<mix_d2*>(__builtin_assume_aligned(row + i + 2, 16)) = mix_d2{a2, a3};
        }
    } else {
        if (i >= 0) row[i] = (OUT)a0;
        if (i + 1 >= 0 && i + 1 < L) row[i + 1] = (OUT)a1;
        if (i + 2 >= 0 && i + 2 < L) row[i + 2] = (OUT)a2;
        if (i + 3 >= 0 && i + 3 < L) row[i + 3] = (OUT)a3;
    }
}

}  // namespace

extern "C" int tt_mix_tile(void) { return MIX_TILE; }
extern "C" int tt_mix_targets_tile(void) { return MIX_TILE; }

extern "C" int tt_mix_audio(const float* arena, const int64_t* tracks, int n_tracks, const int* stem_track, const int64_t* stem_start,
                            const int* item_off, const int* item_split, int B, int64_t N, float* y, void* stream) {
    if (B < 0 || N < 0 || n_tracks < 0) return TT_E_BADARG;
    if (B == 0 || N == 0) return 0;
    if (!item_off || !item_split || !y || (n_tracks > 0 && (!arena || !tracks))) return TT_E_BADARG;
    // a row's first quad begins up to 3 elements in front of it: at most one tile more than N / MIX_TILE for every row
    const long tiles = mix_tiles((long)N, 3);
    if (tiles * (long)B > 0x7fffffffL) return TT_E_BADARG;
    hipLaunchKernelGGL(k_mix_audio, dim3((unsigned)(tiles * B)), dim3(MIX_THREADS), 0, tt_stream(stream), arena,
                       reinterpret_cast<const long*>(tracks), n_tracks, stem_track, reinterpret_cast<const long*>(stem_start), item_off,
                       item_split, (long)N, tiles, y);
    TT_LAUNCH_CHECK();
    return 0;
}

extern "C" int tt_mix_targets(const double* maps, const int* item_off, int B, int F, int64_t T, int out_float32, void* out, void* stream) {
    if (B < 0 || F < 0 || T < 0) return TT_E_BADARG;
    const long L = (long)F * (long)T;
    if (B == 0 || L == 0) return 0;
    if (!item_off || !out) return TT_E_BADARG;
    const long tiles = mix_tiles(L, 3);
    if (tiles * (long)B > 0x7fffffffL) return TT_E_BADARG;
    const dim3 grid((unsigned)(tiles * B));
    if (out_float32)
        hipLaunchKernelGGL(k_mix_targets<float>, grid, dim3(MIX_THREADS), 0, tt_stream(stream), maps, item_off, L, tiles,
                           static_cast<float*>(out));
    else
        hipLaunchKernelGGL(k_mix_targets<double>, grid, dim3(MIX_THREADS), 0, tt_stream(stream), maps, item_off, L, tiles,
                           static_cast<double*>(out));
    TT_LAUNCH_CHECK();
    return 0;
}
