// Per-frame pitch contours and pitch bends of note events on the device (include/ttrap.h: tt_contours_*): integers, exact fp32 values
// and float64 values formed by a fixed sequence of individually rounded operations; no atomics, no environment switches.  The
// semantics are stated in the header; this file is their only device form and tests/contours_ref.py their NumPy restatement.
//
//   x (B, F, T) fp32 + the notes tt_events_fill wrote --k_contours_notes--> per frame of every note: bin, delta, value, pitch, bend
//                                                                            per note: n_voiced, bend_sum, bend_min, bend_max
//   x (F, T) fp32 + the per-frame bin lists of tt_mpe_fill --k_contours_frames--> per list entry: delta, pitch
//
// k_contours_notes: one wavefront per note, lanes along t in chunks of 64 frames, so every load of a row of x is 64 adjacent floats.
// A lane walks the bins of the note's row with the value above and below carried in registers (as k_events_mask does), keeps the
// largest passing value (ties: the lowest bin) together with ITS two neighbours, refines once per frame, and carries the four per-note
// results across the chunks; one integer wave reduction per note ends it.  Slots of a note beyond its (clamped) frames -- reachable
// only with arrays tt_events_fill did not write -- receive the values of an unvoiced frame, so every slot below frame_off[n_notes] is
// written whatever the operands hold.
// k_contours_frames: one lane per frame, walking est_off[t] .. est_off[t + 1]; neighbouring lanes read neighbouring t of the rows
// their bins name.
//
// Every offset into x and the outputs is 64-bit; the grids are one-dimensional with a grid-stride loop.
#include "common.h"

// refine() rounds a - c, (a - b) + (c - b), the quotient, its half and delta * step separately, and the restatement does the same in
// NumPy scalars: nothing in this file may be contracted into a fused multiply-add.  The quotient is the IEEE divide (this file is
// built without fast-math flags and must stay so, like resample.hip).
#pragma clang fp contract(off)

#define CT_WAVES 4                              // wavefronts per workgroup of k_contours_notes
#define CT_MAX_BLOCKS (1 << 20)                 // grid cap; the kernels stride over the rest
#define CT_BEND_LIMIT 1073741824.0              // 2^30

namespace {

__device__ __forceinline__ bool ct_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool ct_finite_d(double v) {
    return ((unsigned long long)__double_as_longlong(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// delta of the triple (a below, b at the bin, c above), each operation rounded on its own
__device__ __forceinline__ float ct_delta(float a, float b, float c) {
    if (!(ct_finite(a) && ct_finite(b) && ct_finite(c) && b >= a && b >= c)) return 0.f;
    const float num = a - c;
    const float den = (a - b) + (c - b);
    float d = 0.f;
    if (den < 0.f) {
        const float q = num / den;
        d = 0.5f * q;
    }
    if (d != d) d = 0.f;                        // inf / inf, where a - c and the curvature both overflow
    if (d < -0.5f) d = -0.5f;
    if (d > 0.5f) d = 0.5f;
    return d;
}

// m[f] + delta * (spacing towards the side delta points to; the other side's where that neighbour does not exist; 0 at F = 1)
__device__ __forceinline__ double ct_pitch(const double* __restrict__ m, int f, int F, float delta) {
    const double mf = m[f];
    double step = 0.0;
    if (F > 1) {
        const bool up = delta >= 0.f ? f + 1 < F : f == 0;
        step = up ? m[f + 1] - mf : mf - m[f - 1];
    }
    const double move = (double)delta * step;
    return mf + move;
}

__device__ __forceinline__ int ct_bend(double pitch, double row_pitch, double units) {
    const double diff = pitch - row_pitch;
    const double prod = diff * units;
    if (!ct_finite_d(prod)) return 0;
    double r = rint(prod);                      // ties to even
    r = r < -CT_BEND_LIMIT ? -CT_BEND_LIMIT : (r > CT_BEND_LIMIT ? CT_BEND_LIMIT : r);
    return (int)r;
}

__device__ __forceinline__ void ct_group(const int* __restrict__ group_off, long p, int F, int& g0, int& g1) {
    g0 = group_off[p];
    g1 = group_off[p + 1];
    g0 = g0 < 0 ? 0 : (g0 > F ? F : g0);        // a table outside [0, F] must never turn into an address
    g1 = g1 < g0 ? g0 : (g1 > F ? F : g1);
}

__global__ __launch_bounds__(64 * CT_WAVES) void k_contours_notes(
    const float* __restrict__ x, long B, int F, int T, double thr, int mode, int fv, const int* __restrict__ group_off, int P,
    const double* __restrict__ m, const double* __restrict__ row_pitch, double units, const int* __restrict__ item,
    const int* __restrict__ row_in, const int* __restrict__ onset, const int* __restrict__ end_in, long n_notes,
    const long* __restrict__ frame_off, int* __restrict__ bin_out, float* __restrict__ delta_out, float* __restrict__ value_out,
    double* __restrict__ pitch_out, int* __restrict__ bend_out, int* __restrict__ n_voiced, long* __restrict__ bend_sum,
    int* __restrict__ bend_min, int* __restrict__ bend_max) {
    const int lane = threadIdx.x & 63;
    const double quiet_nan = __longlong_as_double(0x7ff8000000000000ll);
    long total = frame_off[n_notes];
    total = total < 0 ? 0 : total;
    for (long i = (long)blockIdx.x * CT_WAVES + (threadIdx.x >> 6); i < n_notes; i += (long)gridDim.x * CT_WAVES) {
        long b = item[i], p = row_in[i];
        int t0 = onset[i], t1 = end_in[i];
        // the arrays come from tt_events_fill; whatever else they hold is clamped into the map and reads as an empty note
        b = b < 0 ? 0 : (b >= B ? B - 1 : b);
        p = p < 0 ? 0 : (p >= P ? P - 1 : p);
        t0 = t0 < 0 ? 0 : (t0 > T ? T : t0);
        t1 = t1 < t0 ? t0 : (t1 > T ? T : t1);
        long lo = frame_off[i], hi = frame_off[i + 1];
        lo = lo < 0 ? 0 : (lo > total ? total : lo);        // the slots of the note, inside the arrays
        hi = hi < lo ? lo : (hi > total ? total : hi);
        int g0, g1;
        ct_group(group_off, p, F, g0, g1);
        const float* __restrict__ xb = x + b * F * (long)T;
        const double rp = row_pitch[p];
        int voiced = 0, bmin = 0x7fffffff, bmax = -0x7fffffff - 1;
        long bsum = 0;
        for (long k = lane; k < hi - lo; k += 64) {
            const long t = (long)t0 + k;
            int best_f = -1;
            float best = 0.f, best_a = 0.f, best_c = 0.f;
            if (t < t1 && g1 > g0) {
                const float* __restrict__ col = xb + t;
                auto rd = [&](int f) { return f >= 0 && f < fv ? col[(long)f * T] : 0.f; };
                float up = rd(g0 - 1), cur = rd(g0);
                for (int f = g0; f < g1; ++f) {
                    const float dn = rd(f + 1);
                    if (tt_pick_pass(cur, up, dn, thr, mode) && (best_f < 0 || cur > best)) {
                        best_f = f;
                        best = cur;
                        best_a = up;
                        best_c = dn;
                    }
                    up = cur;
                    cur = dn;
                }
            }
            float d = 0.f;
            double pt = quiet_nan;
            int bd = 0;
            if (best_f >= 0) {
                d = ct_delta(best_a, best, best_c);
                pt = ct_pitch(m, best_f, F, d);
                bd = ct_bend(pt, rp, units);
                ++voiced;
                bsum += bd;
                bmin = bd < bmin ? bd : bmin;
                bmax = bd > bmax ? bd : bmax;
            }
            bin_out[lo + k] = best_f;
            delta_out[lo + k] = d;
            value_out[lo + k] = best;
            pitch_out[lo + k] = pt;
            bend_out[lo + k] = bd;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            voiced += __shfl_xor(voiced, o, 64);
            bsum += __shfl_xor(bsum, o, 64);
            const int omin = __shfl_xor(bmin, o, 64), omax = __shfl_xor(bmax, o, 64);
            bmin = omin < bmin ? omin : bmin;
            bmax = omax > bmax ? omax : bmax;
        }
        if (lane == 0) {
            n_voiced[i] = voiced;
            bend_sum[i] = bsum;
            bend_min[i] = voiced ? bmin : 0;
            bend_max[i] = voiced ? bmax : 0;
        }
    }
}

__global__ __launch_bounds__(256) void k_contours_frames(const float* __restrict__ x, int F, int T, int fv, const long* __restrict__ est_off,
                                                         const int* __restrict__ est_bins, long cap, const double* __restrict__ m,
                                                         float* __restrict__ delta_out, double* __restrict__ pitch_out) {
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < T; t += (long)gridDim.x * 256) {
        long j0 = est_off[t], j1 = est_off[t + 1];
        j0 = j0 < 0 ? 0 : j0;
        j1 = j1 > cap ? cap : j1;               // nothing at or beyond the capacity
        const float* __restrict__ col = x + t;
        for (long j = j0; j < j1; ++j) {
            int f = est_bins[j];
            f = f < 0 ? 0 : (f >= F ? F - 1 : f);           // a list that names no bin of the map must never turn into an address
            auto rd = [&](int g) { return g >= 0 && g < fv ? col[(long)g * T] : 0.f; };
            const float d = ct_delta(rd(f - 1), col[(long)f * T], rd(f + 1));
            delta_out[j] = d;
            pitch_out[j] = ct_pitch(m, f, F, d);
        }
    }
}

inline int ct_fv(int F, int f_valid) { return f_valid > 0 && f_valid < F ? f_valid : F; }
inline unsigned ct_grid(long items, int per_block) {
    const long blocks = (items + per_block - 1) / per_block;
    return (unsigned)(blocks < 1 ? 1 : (blocks > CT_MAX_BLOCKS ? CT_MAX_BLOCKS : blocks));
}

}  // namespace

extern "C" int tt_contours_notes(const float* x, int B, int F, int T, double threshold, int mode, int f_valid, const int* group_off, int P,
                                 const double* m, const double* row_pitch, int units, const int* item, const int* row, const int* onset,
                                 const int* end, int64_t n_notes, const int64_t* frame_off, int* bin, float* delta, float* value,
                                 double* pitch, int* bend, int* n_voiced, int64_t* bend_sum, int* bend_min, int* bend_max, void* stream) {
    if (!x || !group_off || B < 1 || F < 1 || T < 1 || P < 1 || (mode != 1 && mode != 2) || !m || !row_pitch || units < 1 || !item || !row ||
        !onset || !end || n_notes < 1 || !frame_off || !bin || !delta || !value || !pitch || !bend || !n_voiced || !bend_sum || !bend_min ||
        !bend_max)
        return TT_E_BADARG;
    hipLaunchKernelGGL(k_contours_notes, dim3(ct_grid((long)n_notes, CT_WAVES)), dim3(64 * CT_WAVES), 0, tt_stream(stream), x, (long)B, F, T,
                       threshold, mode, ct_fv(F, f_valid), group_off, P, m, row_pitch, (double)units, item, row, onset, end, (long)n_notes,
                       reinterpret_cast<const long*>(frame_off), bin, delta, value, pitch, bend, n_voiced, reinterpret_cast<long*>(bend_sum),
                       bend_min, bend_max);
    TT_LAUNCH_CHECK();
    return 0;
}

extern "C" int tt_contours_frames(const float* x, int F, int T, int f_valid, const int64_t* est_off, const int* est_bins, int64_t capacity,
                                  const double* m, float* delta, double* pitch, void* stream) {
    if (!x || F < 1 || T < 1 || !est_off || !est_bins || capacity < 0 || !m || !delta || !pitch) return TT_E_BADARG;
    hipLaunchKernelGGL(k_contours_frames, dim3(ct_grid((long)T, 256)), dim3(256), 0, tt_stream(stream), x, F, T, ct_fv(F, f_valid),
                       reinterpret_cast<const long*>(est_off), est_bins, (long)capacity, m, delta, pitch);
    TT_LAUNCH_CHECK();
    return 0;
}
