// Multi-pitch scoring on the device (include/ttrap.h: tt_mpe_*): integers and float64 comparisons only, no atomics, no recursion.
//
//   activations (F, T) fp32 --k_mpe_compact<false>--> n_est[T] --(prefix sum, caller)--> est_off[T + 1]
//                           --k_mpe_compact<true>---> est_bins[est_off[t] .. est_off[t + 1])   (active bins of frame t, ascending)
//   reference frame j reads estimate frame est_idx[j] --k_mpe_match--> tp[j], tp_chroma[j], n_est[j]
//
// k_mpe_compact: one lane per frame walking down F (adjacent lanes read adjacent floats of a row: coalesced), MPE_ROWS rows loaded ahead of
// the compares.  The predicate is k_peak_pick's (losses.hip) mode 1 / mode 2, expression for expression: rows f >= f_valid read as zero,
// strict local maximum against zeros beyond both ends, (double)v >= threshold.
//
// k_mpe_match: one wavefront (= one workgroup) per reference frame.  Lane l holds the MIDI values of estimates l, l + 64, l + 128, l + 192
// in registers; for every reference pitch the 64 lanes evaluate |r - e| <= window (and the octave-wrapped distance for the chroma scores)
// and __ballot hands the 64 verdicts back as one word of the adjacency bit row in LDS.  Lanes 0 and 1 then run Kuhn's augmenting-path
// search -- lane 0 on the plain rows, lane 1 on the chroma rows, same code, so the two searches share their instructions -- iteratively:
// an explicit stack of (reference, chosen estimate) pairs and a `seen` bit mask per search root.  Every reference on the stack is distinct
// (the root is unmatched, the others are the partners of distinct estimates), so the stack never holds more than n_ref <= MPE_MAX_REF
// entries.  The size of a maximum matching is unique, so the order in which candidates are tried cannot change the count.
#include "common.h"
#include <math.h>

#define MPE_MAX_EST 256                         // = tt_mpe_max_est(): active bins per frame the matcher holds (>= 236, the most strict peaks 472 bins can hold)
#define MPE_MAX_REF 64                          // = tt_mpe_max_ref(): reference pitches per frame
#define MPE_WORDS (MPE_MAX_EST / 64)
#define MPE_ROWS 8                              // rows of the activation map a lane loads ahead

static_assert(MPE_MAX_EST % 64 == 0 && MPE_MAX_EST <= 32767 && MPE_MAX_REF <= 32767, "bit rows of whole words; indices fit a short");

namespace {

template <bool FILL>
__global__ __launch_bounds__(64) void k_mpe_compact(const float* __restrict__ x, int F, int T, double thr, int mode, int fv,
                                                    const unsigned char* __restrict__ bin_bad, const long* __restrict__ est_off, long cap,
                                                    int* __restrict__ n_est, int* __restrict__ bad_out, int* __restrict__ est_bins) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= T) return;
    const float* __restrict__ col = x + t;
    const long w0 = FILL ? est_off[t] : 0;
    int n = 0, bad = 0;
    auto emit = [&](int f) {
        if (FILL) {
            if (w0 + n < cap) est_bins[w0 + n] = f;
        } else if (bin_bad) {
            bad |= bin_bad[f];
        }
        ++n;
    };
    float up = 0.f, cur = col[0];
    for (int f0 = 0; f0 < fv; f0 += MPE_ROWS) {
        float nx[MPE_ROWS];
#pragma unroll
        for (int i = 0; i < MPE_ROWS; ++i) {
            const int f = f0 + i + 1;
            nx[i] = f < fv ? col[(long)f * T] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < MPE_ROWS; ++i) {
            const int f = f0 + i;
            if (f < fv) {
                if (tt_pick_pass(cur, up, nx[i], thr, mode)) emit(f);
                up = cur;
                cur = nx[i];
            }
        }
    }
    if (mode == 1 && 0.0 >= thr)                // the masked rows read as zero, and zero reaches a threshold <= 0
        for (int f = fv; f < F; ++f) emit(f);
    if (!FILL) {
        n_est[t] = n;
        bad_out[t] = bad;
    }
}

__global__ __launch_bounds__(64) void k_mpe_match(const int* __restrict__ est_idx, int T, const long* __restrict__ est_off,
                                                  const int* __restrict__ est_bins, const double* __restrict__ est_midi, int F,
                                                  const long* __restrict__ ref_off, const double* __restrict__ ref_midi, double window,
                                                  int* __restrict__ tp, int* __restrict__ tp_chroma, int* __restrict__ n_est_out) {
    __shared__ unsigned long long adj[2][MPE_MAX_REF][MPE_WORDS];
    __shared__ short match[2][MPE_MAX_EST];
    __shared__ short stk_r[2][MPE_MAX_REF], stk_e[2][MPE_MAX_REF];
    const long j = blockIdx.x;
    const int lane = threadIdx.x;
    const int ei = est_idx[j];
    const long r0 = ref_off[j], nr_l = ref_off[j + 1] - r0;
    long e0 = 0, ne_l = 0;
    if (ei >= 0 && ei < T) {
        e0 = est_off[ei];
        ne_l = est_off[ei + 1] - e0;
    }
    if (nr_l > MPE_MAX_REF || ne_l > MPE_MAX_EST) {         // over a capacity: flagged, nothing else written, no LDS touched
        if (lane == 0) tp[j] = -1;
        return;
    }
    if (nr_l <= 0 || ne_l <= 0) {
        if (lane == 0) {
            tp[j] = 0;
            tp_chroma[j] = 0;
            n_est_out[j] = ne_l > 0 ? (int)ne_l : 0;
        }
        return;
    }
    const int nr = (int)nr_l, ne = (int)ne_l;
    double ev[MPE_WORDS], ec[MPE_WORDS];
#pragma unroll
    for (int w = 0; w < MPE_WORDS; ++w) {
        const int e = w * 64 + lane;
        int b = e < ne ? est_bins[e0 + e] : 0;
        b = b < 0 ? 0 : (b >= F ? F - 1 : b);
        ev[w] = est_midi[b];
        ec[w] = fmod(ev[w], 12.0);
        match[0][e] = -1;
        match[1][e] = -1;
    }
    for (int r = 0; r < nr; ++r) {
        const double rv = ref_midi[r0 + r], rc = fmod(rv, 12.0);
#pragma unroll
        for (int w = 0; w < MPE_WORDS; ++w) {
            const bool live = w * 64 + lane < ne;
            const double d = fmod(fabs(rc - ec[w]), 12.0), d2 = 12.0 - d;
            const unsigned long long plain = __ballot(live && fabs(rv - ev[w]) <= window);
            const unsigned long long chroma = __ballot(live && (d < d2 ? d : d2) <= window);
            if (lane == 0) {
                adj[0][r][w] = plain;
                adj[1][r][w] = chroma;
            }
        }
    }
    __syncthreads();
    if (lane >= 2) return;
    const int c = lane;
    int count = 0;
    for (int root = 0; root < nr; ++root) {
        unsigned long long seen[MPE_WORDS];
#pragma unroll
        for (int w = 0; w < MPE_WORDS; ++w) seen[w] = 0ull;
        int sp = 0;
        stk_r[c][0] = (short)root;
        while (sp >= 0) {
            const int r = stk_r[c][sp];
            int e = -1;
#pragma unroll
            for (int w = 0; w < MPE_WORDS; ++w) {
                const unsigned long long m = adj[c][r][w] & ~seen[w];
                if (e < 0 && m) {
                    const int bit = __ffsll((long long)m) - 1;
                    e = w * 64 + bit;
                    seen[w] |= 1ull << bit;
                }
            }
            if (e < 0) {                                    // r has no untried estimate left: back to its caller
                --sp;
                continue;
            }
            stk_e[c][sp] = (short)e;
            const int partner = match[c][e];
            if (partner < 0) {                              // a free estimate: flip the path
                for (int k = sp; k >= 0; --k) match[c][stk_e[c][k]] = stk_r[c][k];
                ++count;
                break;
            }
            if (sp + 1 < MPE_MAX_REF) stk_r[c][++sp] = (short)partner;
            else break;                                     // cannot happen (distinct references on the stack); never write past it
        }
    }
    if (c == 0) {
        tp[j] = count;
        n_est_out[j] = ne;
    } else {
        tp_chroma[j] = count;
    }
}

inline bool mpe_compact_ok(const float* x, int F, int T, int mode) { return x && F >= 1 && T >= 1 && (mode == 1 || mode == 2); }
inline int mpe_fv(int F, int f_valid) { return f_valid > 0 && f_valid < F ? f_valid : F; }

}  // namespace

extern "C" int tt_mpe_max_est(void) { return MPE_MAX_EST; }
extern "C" int tt_mpe_max_ref(void) { return MPE_MAX_REF; }

extern "C" int tt_mpe_count(const float* x, int F, int T, double threshold, int mode, int f_valid, const unsigned char* bin_bad, int* n_est,
                            int* bad_out, void* stream) {
    if (!mpe_compact_ok(x, F, T, mode) || !n_est || !bad_out) return TT_E_BADARG;
    hipLaunchKernelGGL(k_mpe_compact<false>, dim3((T + 63) / 64), dim3(64), 0, tt_stream(stream), x, F, T, threshold, mode, mpe_fv(F, f_valid),
                       bin_bad, (const long*)nullptr, 0L, n_est, bad_out, (int*)nullptr);
    TT_LAUNCH_CHECK();
    return 0;
}

extern "C" int tt_mpe_fill(const float* x, int F, int T, double threshold, int mode, int f_valid, const int64_t* est_off, int64_t capacity,
                           int* est_bins, void* stream) {
    if (!mpe_compact_ok(x, F, T, mode) || !est_off || !est_bins || capacity < 0) return TT_E_BADARG;
    hipLaunchKernelGGL(k_mpe_compact<true>, dim3((T + 63) / 64), dim3(64), 0, tt_stream(stream), x, F, T, threshold, mode, mpe_fv(F, f_valid),
                       (const unsigned char*)nullptr, reinterpret_cast<const long*>(est_off), (long)capacity, (int*)nullptr, (int*)nullptr,
                       est_bins);
    TT_LAUNCH_CHECK();
    return 0;
}

extern "C" int tt_mpe_match(const int* est_idx, int n_ref_frames, int T, const int64_t* est_off, const int* est_bins, const double* est_midi,
                            int F, const int64_t* ref_off, const double* ref_midi, double window, int* tp, int* tp_chroma, int* n_est,
                            void* stream) {
    if (!est_idx || n_ref_frames < 1 || T < 1 || F < 1 || !est_off || !est_bins || !est_midi || !ref_off || !ref_midi || !tp || !tp_chroma ||
        !n_est)
        return TT_E_BADARG;
    hipLaunchKernelGGL(k_mpe_match, dim3(n_ref_frames), dim3(64), 0, tt_stream(stream), est_idx, T, reinterpret_cast<const long*>(est_off),
                       est_bins, est_midi, F, reinterpret_cast<const long*>(ref_off), ref_midi, window, tp, tp_chroma, n_est);
    TT_LAUNCH_CHECK();
    return 0;
}
