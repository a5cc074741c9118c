// Note events from activation maps on the device (include/ttrap.h: tt_events_*): bit words, integers and exact fp32 maxima only, no
// atomics, no environment switches; the way back from csrc/notes.hip (notes -> frames).
//
//   x (B, F, T) fp32 --k_events_mask--> a[B][P][W] 64-bit words, W = ceil(T / 64): bit i of word w = frame 64 w + i of pitch row p is active
//                    --k_events_count--> n_on[B][P][W], n_end[B][P][W]   --(two exclusive prefix sums, caller)--> on_off, end_off
//                    --k_events_fill---> item / row / onset of candidate on_off + rank, end (exclusive) of candidate end_off + rank
//                    --k_events_finish-> n_active, peak, keep per candidate
//
// Pitch row p owns the bins [group_off[p], group_off[p + 1]); a frame of the row is active when one of its bins passes tt_pick_pass
// (common.h: the predicate of tt_peak_pick / tt_mpe_count), evaluated on rows that read as zero from f_valid upwards and beyond both ends.
//
// k_events_mask: one wavefront per word, lanes along t, so every load of a row of x is 64 adjacent floats; the wave walks the row's bins
// with the value above and below carried in registers, and __ballot hands the 64 verdicts back as the word.  Bits beyond T are zero.
//
// Runs.  With G = max_gap, a gap of at most G zeros between two ones is filled, so the ones of a row fall into notes: an active frame t
// opens a note iff none of the G + 1 frames before it is active, and closes one iff none of the G + 1 frames after it is.  Per word,
// on 128-bit values (the previous word below the current one; the current one below the next), that is
//     on  = a & ~(a << 1 | a << 2 | ... | a << (G + 1))        end = a & ~(a >> 1 | ... | a >> (G + 1))
// with the OR of G + 1 shifts formed by doubling (ev_smear: 1, 2, 4, ... shifts OR-ed onto themselves, at most seven steps).  Only the
// two neighbouring words OF THE SAME ROW are read -- the first and last word of a row see zeros beyond it, so a row never merges with the
// next row or item.  Every note has exactly one opening and one closing frame, the i-th opening of a row belongs with its i-th closing,
// and the per-row totals of the two counts are equal: the two prefix sums therefore index the same candidate slots.
//
// k_events_count / k_events_fill: one lane per word (they move 8 bytes per 64 frames; the map itself is read by the other two kernels).
// k_events_finish: one wavefront per candidate: popcount of the note's mask words, maximum of x over frames x row bins under the same
// predicate (lanes along t again), both reduced across the wave; keep = the note spans at least min_frames frames.
//
// Every offset into x, the words or the candidate arrays is 64-bit; the grids are one-dimensional with a grid-stride loop, so B P W may
// be any size.
#include "common.h"

#define EV_WAVES 4                              // wavefronts per workgroup of the wave-per-item kernels
#define EV_MAX_BLOCKS (1 << 20)                 // grid cap; the kernels stride over the rest

namespace {

typedef unsigned long long u64;

struct EvWide {                                 // 128 bits
    u64 lo, hi;
};
// shifts by 1 <= k <= 63
__device__ __forceinline__ EvWide ev_shl(EvWide v, int k) { return {v.lo << k, (v.hi << k) | (v.lo >> (64 - k))}; }
__device__ __forceinline__ EvWide ev_shr(EvWide v, int k) { return {(v.lo >> k) | (v.hi << (64 - k)), v.hi >> k}; }
__device__ __forceinline__ EvWide ev_or(EvWide a, EvWide b) { return {a.lo | b.lo, a.hi | b.hi}; }

// OR of v shifted by 1 .. n (1 <= n <= 64), up (UP) or down: r = OR of the shifts 0 .. m - 1 doubles m while 2 m <= n, one more OR with
// r shifted by n - m <= m completes the window, and the whole moves by one.
template <bool UP>
__device__ __forceinline__ EvWide ev_smear(EvWide v, int n) {
    EvWide r = v;
    int m = 1;
    while (2 * m <= n) {
        r = ev_or(r, UP ? ev_shl(r, m) : ev_shr(r, m));
        m *= 2;
    }
    if (n > m) r = ev_or(r, UP ? ev_shl(r, n - m) : ev_shr(r, n - m));
    return UP ? ev_shl(r, 1) : ev_shr(r, 1);
}

// opening and closing frames of word w of one row (row: its W words)
__device__ __forceinline__ void ev_edges(const u64* __restrict__ row, long w, long W, int gap, u64& on, u64& end) {
    const u64 cur = row[w];
    const u64 prev = w > 0 ? row[w - 1] : 0ull, next = w + 1 < W ? row[w + 1] : 0ull;
    on = cur & ~ev_smear<true>({prev, cur}, gap + 1).hi;
    end = cur & ~ev_smear<false>({cur, next}, gap + 1).lo;
}

// the bins [g0, g1) of frame t of one item (col = x + b F T + t): does one pass; the largest value among those that do
__device__ __forceinline__ bool ev_row_pass(const float* __restrict__ col, long T, int g0, int g1, int fv, double thr, int mode, float& best) {
    auto rd = [&](int f) { return f >= 0 && f < fv ? col[(long)f * T] : 0.f; };
    bool any = false;
    float up = rd(g0 - 1), cur = rd(g0);
    for (int f = g0; f < g1; ++f) {
        const float dn = rd(f + 1);
        if (tt_pick_pass(cur, up, dn, thr, mode)) {
            best = any ? (cur > best ? cur : best) : cur;
            any = true;
        }
        up = cur;
        cur = dn;
    }
    return any;
}

__device__ __forceinline__ void ev_group(const int* __restrict__ group_off, long p, int F, int& g0, int& g1) {
    g0 = group_off[p];
    g1 = group_off[p + 1];
    g0 = g0 < 0 ? 0 : (g0 > F ? F : g0);        // a table outside [0, F] must never turn into an address
    g1 = g1 < g0 ? g0 : (g1 > F ? F : g1);
}

__global__ __launch_bounds__(64 * EV_WAVES) void k_events_mask(const float* __restrict__ x, long B, int F, int T, double thr, int mode, int fv,
                                                               const int* __restrict__ group_off, int P, long W, u64* __restrict__ mask) {
    const int lane = threadIdx.x & 63;
    const long n = B * P * W;
    for (long i = (long)blockIdx.x * EV_WAVES + (threadIdx.x >> 6); i < n; i += (long)gridDim.x * EV_WAVES) {
        const long w = i % W, p = (i / W) % P, b = i / (W * P);
        int g0, g1;
        ev_group(group_off, p, F, g0, g1);
        const long t = w * 64 + lane;
        bool any = false;
        float best = 0.f;
        if (t < T && g1 > g0) any = ev_row_pass(x + b * F * (long)T + t, T, g0, g1, fv, thr, mode, best);
        const u64 word = __ballot(any);
        if (lane == 0) mask[i] = word;
    }
}

template <bool FILL>
__global__ __launch_bounds__(256) void k_events_edges(const u64* __restrict__ mask, long rows, long W, int P, int gap, int* __restrict__ n_on,
                                                      int* __restrict__ n_end, const long* __restrict__ on_off,
                                                      const long* __restrict__ end_off, long cap, int* __restrict__ item, int* __restrict__ row_out,
                                                      int* __restrict__ onset, int* __restrict__ end_out) {
    const long n = rows * W;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const long r = i / W, w = i - r * W;
        u64 on, end;
        ev_edges(mask + r * W, w, W, gap, on, end);
        if (!FILL) {
            n_on[i] = __popcll(on);
            n_end[i] = __popcll(end);
            continue;
        }
        const int base = (int)(w * 64);
        for (long s = on_off[i]; on; on &= on - 1, ++s) {
            if (s >= cap) break;
            item[s] = (int)(r / P);
            row_out[s] = (int)(r % P);
            onset[s] = base + __ffsll((long long)on) - 1;
        }
        for (long s = end_off[i]; end; end &= end - 1, ++s) {
            if (s >= cap) break;
            end_out[s] = base + __ffsll((long long)end);            // exclusive
        }
    }
}

__global__ __launch_bounds__(64 * EV_WAVES) void k_events_finish(const float* __restrict__ x, long B, int F, int T, double thr, int mode, int fv,
                                                                 const int* __restrict__ group_off, int P, long W, const u64* __restrict__ mask,
                                                                 const int* __restrict__ item, const int* __restrict__ row_in,
                                                                 const int* __restrict__ onset, const int* __restrict__ end_in, long n_notes,
                                                                 int min_frames, int* __restrict__ n_active, float* __restrict__ peak,
                                                                 int* __restrict__ keep) {
    const int lane = threadIdx.x & 63;
    for (long i = (long)blockIdx.x * EV_WAVES + (threadIdx.x >> 6); i < n_notes; i += (long)gridDim.x * EV_WAVES) {
        long b = item[i], p = row_in[i];
        int t0 = onset[i], t1 = end_in[i];
        // candidates come from tt_events_fill; whatever else the arrays hold is clamped into the map and reads as an empty note
        b = b < 0 ? 0 : (b >= B ? B - 1 : b);
        p = p < 0 ? 0 : (p >= P ? P - 1 : p);
        t0 = t0 < 0 ? 0 : (t0 > T ? T : t0);
        t1 = t1 < t0 ? t0 : (t1 > T ? T : t1);
        int g0, g1;
        ev_group(group_off, p, F, g0, g1);
        const u64* __restrict__ words = mask + (b * P + p) * W;
        const float* __restrict__ xb = x + b * F * (long)T;
        int count = 0;
        bool any = false;
        float best = 0.f;
        if (t1 > t0) {
            const long w0 = t0 >> 6, w1 = (t1 - 1) >> 6;
            for (long w = w0 + lane; w <= w1; w += 64) {
                u64 m = words[w];
                if (w == w0) m &= ~0ull << (t0 & 63);
                if (w == w1 && (t1 & 63)) m &= ~0ull >> (64 - (t1 & 63));
                count += __popcll(m);
            }
            for (long w = w0; w <= w1; ++w) {
                const long t = w * 64 + lane;
                float v = 0.f;
                if (t >= t0 && t < t1 && g1 > g0 && ev_row_pass(xb + t, T, g0, g1, fv, thr, mode, v)) {
                    best = any ? (v > best ? v : best) : v;
                    any = true;
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            count += __shfl_xor(count, o, 64);
            const float ob = __shfl_xor(best, o, 64);
            const bool oa = __shfl_xor((int)any, o, 64) != 0;
            if (oa) {
                best = any ? (ob > best ? ob : best) : ob;
                any = true;
            }
        }
        if (lane == 0) {
            n_active[i] = count;
            peak[i] = best;
            keep[i] = (t1 - t0 >= min_frames) ? 1 : 0;
        }
    }
}

inline bool ev_map_ok(const float* x, int B, int F, int T, int mode, const int* group_off, int P) {
    return x && group_off && B >= 1 && F >= 1 && T >= 1 && P >= 1 && (mode == 1 || mode == 2);
}
inline bool ev_gap_ok(int max_gap) { return max_gap >= 0 && max_gap <= 63; }
inline int ev_fv(int F, int f_valid) { return f_valid > 0 && f_valid < F ? f_valid : F; }
inline long ev_words(int T) { return ((long)T + 63) / 64; }
inline unsigned ev_grid(long items, int per_block) {
    const long blocks = (items + per_block - 1) / per_block;
    return (unsigned)(blocks < 1 ? 1 : (blocks > EV_MAX_BLOCKS ? EV_MAX_BLOCKS : blocks));
}

}  // namespace

extern "C" int tt_events_mask(const float* x, int B, int F, int T, double threshold, int mode, int f_valid, const int* group_off, int P,
                              uint64_t* mask, void* stream) {
    if (!ev_map_ok(x, B, F, T, mode, group_off, P) || !mask) return TT_E_BADARG;
    const long W = ev_words(T);
    hipLaunchKernelGGL(k_events_mask, dim3(ev_grid((long)B * P * W, EV_WAVES)), dim3(64 * EV_WAVES), 0, tt_stream(stream), x, (long)B, F, T,
                       threshold, mode, ev_fv(F, f_valid), group_off, P, W, reinterpret_cast<u64*>(mask));
    TT_LAUNCH_CHECK();
    return 0;
}

extern "C" int tt_events_count(const uint64_t* mask, int B, int P, int T, int max_gap, int* n_on, int* n_end, void* stream) {
    if (!mask || B < 1 || P < 1 || T < 1 || !ev_gap_ok(max_gap) || !n_on || !n_end) return TT_E_BADARG;
    const long W = ev_words(T), rows = (long)B * P;
    hipLaunchKernelGGL(k_events_edges<false>, dim3(ev_grid(rows * W, 256)), dim3(256), 0, tt_stream(stream), reinterpret_cast<const u64*>(mask),
                       rows, W, P, max_gap, n_on, n_end, (const long*)nullptr, (const long*)nullptr, 0L, (int*)nullptr, (int*)nullptr,
                       (int*)nullptr, (int*)nullptr);
    TT_LAUNCH_CHECK();
    return 0;
}

extern "C" int tt_events_fill(const uint64_t* mask, int B, int P, int T, int max_gap, const int64_t* on_off, const int64_t* end_off,
                              int64_t capacity, int* item, int* row, int* onset, int* end, void* stream) {
    if (!mask || B < 1 || P < 1 || T < 1 || !ev_gap_ok(max_gap) || !on_off || !end_off || capacity < 0 || !item || !row || !onset || !end)
        return TT_E_BADARG;
    const long W = ev_words(T), rows = (long)B * P;
    hipLaunchKernelGGL(k_events_edges<true>, dim3(ev_grid(rows * W, 256)), dim3(256), 0, tt_stream(stream), reinterpret_cast<const u64*>(mask),
                       rows, W, P, max_gap, (int*)nullptr, (int*)nullptr, reinterpret_cast<const long*>(on_off),
                       reinterpret_cast<const long*>(end_off), (long)capacity, item, row, onset, end);
    TT_LAUNCH_CHECK();
    return 0;
}

extern "C" int tt_events_finish(const float* x, int B, int F, int T, double threshold, int mode, int f_valid, const int* group_off, int P,
                                const uint64_t* mask, const int* item, const int* row, const int* onset, const int* end, int64_t n_notes,
                                int min_frames, int* n_active, float* peak, int* keep, void* stream) {
    if (!ev_map_ok(x, B, F, T, mode, group_off, P) || !mask || !item || !row || !onset || !end || n_notes < 1 || min_frames < 1 || !n_active ||
        !peak || !keep)
        return TT_E_BADARG;
    hipLaunchKernelGGL(k_events_finish, dim3(ev_grid((long)n_notes, EV_WAVES)), dim3(64 * EV_WAVES), 0, tt_stream(stream), x, (long)B, F, T,
                       threshold, mode, ev_fv(F, f_valid), group_off, P, ev_words(T), reinterpret_cast<const u64*>(mask), item, row, onset, end,
                       (long)n_notes, min_frames, n_active, peak, keep);
    TT_LAUNCH_CHECK();
    return 0;
}
