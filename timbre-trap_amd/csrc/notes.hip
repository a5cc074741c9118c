// Note annotations to per-frame lists on the device (include/ttrap.h: tt_note_*): integers and float64 comparisons only, no atomics.
//
//   intervals (L, 2) float64, times (N) float64 non-decreasing --k_note_spans--> lo[L], hi[L]   (note i sounds in frames lo[i] <= t < hi[i])
//   lo, hi --k_note_csr<false>--> count[N] --(prefix sum, caller)--> off[N + 1]
//          --k_note_csr<true>---> note_idx[off[t] .. off[t + 1])   (the notes that hold frame t, ascending note index)
//
// k_note_spans: one lane per note, two binary searches over `times` with the reference's own comparisons (`times >= onset`, `times <
// offset`, NoteDataset.py:119) -- on a non-decreasing grid both are prefixes' complements, so the frames of a note are one half-open range.
//
// k_note_csr: one workgroup per tile of NOTE_TILE frames, one lane per frame.  The notes pass through LDS NOTE_CHUNK at a time: lane k of
// the workgroup tests note c0 + k against the TILE (not against a frame), __ballot and a popcount of the lower lanes give every
// overlapping note its rank, and the survivors are stored to LDS in note order -- so a chunk of which nothing overlaps the tile costs two
// barriers and no frame loop at all, and the frame loop that does run walks only the tile's own notes.  Every lane then reads the same
// LDS word at a time (a broadcast, no bank conflict) and counts or writes the notes that hold its frame.  Chunks ascend and the
// compaction keeps the order inside a chunk, hence the ascending note order of the lists that the reference's appends give.
#include "common.h"

#define NOTE_TILE 256                           // = tt_note_tile_frames(): frames per workgroup of k_note_csr (one lane each)
#define NOTE_CHUNK 256                          // = tt_note_chunk(): notes tested against a tile per pass (one lane each)

static_assert(NOTE_TILE % 64 == 0 && NOTE_CHUNK == NOTE_TILE, "one lane per frame and per note of a chunk; whole wavefronts");

namespace {

// first index t in [0, N) with !(times[t] < v), N if none: numpy.searchsorted(times, v, side='left') for a v that is not NaN
__device__ __forceinline__ int note_lower_bound(const double* __restrict__ times, int N, double v) {
    int l = 0, h = N;
    while (l < h) {
        const int m = l + ((h - l) >> 1);
        if (times[m] < v) l = m + 1;
        else h = m;
    }
    return l;
}

__global__ __launch_bounds__(256) void k_note_spans(const double* __restrict__ times, int N, const double* __restrict__ iv, int L,
                                                    int* __restrict__ lo, int* __restrict__ hi) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= L) return;
    const double on = iv[2 * (long)i], off = iv[2 * (long)i + 1];
    int a = 0, b = 0;                           // a NaN bound compares false with every frame: an empty range
    if (on == on && off == off) {
        a = note_lower_bound(times, N, on);
        b = note_lower_bound(times, N, off);
    }
    lo[i] = a;
    hi[i] = b;
}

template <bool FILL>
__global__ __launch_bounds__(NOTE_TILE) void k_note_csr(const int* __restrict__ lo, const int* __restrict__ hi, int L, int N,
                                                        const long* __restrict__ off, long cap, int* __restrict__ count,
                                                        int* __restrict__ note_idx) {
    __shared__ int s_lo[NOTE_CHUNK], s_hi[NOTE_CHUNK], s_id[NOTE_CHUNK];
    __shared__ int s_wave[NOTE_TILE / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long t0_l = (long)blockIdx.x * NOTE_TILE;
    const int t0 = (int)t0_l;                                           // < N: the grid holds ceil(N / NOTE_TILE) workgroups
    const int t1 = N - t0 < NOTE_TILE ? N : t0 + NOTE_TILE;
    const int t = t0 + tid;
    const bool live = tid < t1 - t0;                                    // lanes beyond the last frame still stage notes
    const long w0 = (FILL && live) ? off[t] : 0;
    int n = 0;
    for (int c0 = 0; c0 < L; c0 += NOTE_CHUNK) {
        const int i = c0 + tid;
        int a = 0, b = 0;
        if (i < L) {
            a = lo[i];
            b = hi[i];
        }
        const bool hit = i < L && (a > t0 ? a : t0) < (b < t1 ? b : t1);
        const unsigned long long m = __ballot(hit);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();                        // the wave counts are in; and every lane has left the previous chunk's frame loop
        int base = 0, total = 0;
#pragma unroll
        for (int w = 0; w < NOTE_TILE / 64; ++w) {
            const int c = s_wave[w];
            base += w < wave ? c : 0;
            total += c;
        }
        if (hit) {
            const int p = base + __popcll(m & ((1ull << lane) - 1ull));                 // p < total <= NOTE_CHUNK
            s_lo[p] = a;
            s_hi[p] = b;
            s_id[p] = i;
        }
        __syncthreads();                        // the list is in; s_wave is not written again before the next chunk's ballot
        if (live) {
            for (int k = 0; k < total; ++k) {
                if (s_lo[k] <= t && t < s_hi[k]) {
                    if (FILL) {
                        if (w0 + n < cap) note_idx[w0 + n] = s_id[k];
                    }
                    ++n;
                }
            }
        }
    }
    if (!FILL && live) count[t] = n;
}

}  // namespace

extern "C" int tt_note_tile_frames(void) { return NOTE_TILE; }
extern "C" int tt_note_chunk(void) { return NOTE_CHUNK; }

extern "C" int tt_note_spans(const double* times, int N, const double* intervals, int L, int* lo, int* hi, void* stream) {
    if (N < 0 || L < 0 || (N > 0 && !times) || (L > 0 && (!intervals || !lo || !hi))) return TT_E_BADARG;
    if (L == 0) return 0;
    hipLaunchKernelGGL(k_note_spans, dim3((L + 255) / 256), dim3(256), 0, tt_stream(stream), times, N, intervals, L, lo, hi);
    TT_LAUNCH_CHECK();
    return 0;
}

extern "C" int tt_note_count(const int* lo, const int* hi, int L, int N, int* count, void* stream) {
    if (N < 1 || L < 0 || !count || (L > 0 && (!lo || !hi))) return TT_E_BADARG;
    hipLaunchKernelGGL(k_note_csr<false>, dim3((N + NOTE_TILE - 1) / NOTE_TILE), dim3(NOTE_TILE), 0, tt_stream(stream), lo, hi, L, N,
                       (const long*)nullptr, 0L, count, (int*)nullptr);
    TT_LAUNCH_CHECK();
    return 0;
}

extern "C" int tt_note_fill(const int* lo, const int* hi, int L, int N, const int64_t* off, int64_t capacity, int* note_idx, void* stream) {
    if (N < 1 || L < 0 || !off || capacity < 0 || (capacity > 0 && !note_idx) || (L > 0 && (!lo || !hi))) return TT_E_BADARG;
    if (L == 0 || capacity == 0) return 0;
    hipLaunchKernelGGL(k_note_csr<true>, dim3((N + NOTE_TILE - 1) / NOTE_TILE), dim3(NOTE_TILE), 0, tt_stream(stream), lo, hi, L, N,
                       reinterpret_cast<const long*>(off), (long)capacity, (int*)nullptr, note_idx);
    TT_LAUNCH_CHECK();
    return 0;
}
