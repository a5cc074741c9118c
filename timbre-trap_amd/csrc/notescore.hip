// Note-level scoring on the device (include/ttrap.h: tt_notescore_*): integers and float64 comparisons only, no atomics, no recursion,
// every loop with a static bound.  The rule is stated once, in utils/metrics/notescore.py (note_counts); ns_onset_pair / ns_offset_pair below are
// its two predicates, expression for expression.
//
//   notes sorted by (item, onset) on both sides (the caller sorts); node v < R is reference v, node R + k is estimate k
//   k_ns_times    NoteEvents frames -> float64 seconds, the arithmetic of events_to_notes
//   k_ns_ranges   one lane per node: by binary search on the OTHER list, inside the node's item, the contiguous slice [lo, hi) that can
//                 hold partners (onset window widened by 1e-4: rnd(d) <= tol implies d <= tol + 0.5e-4)
//   k_ns_labels   one round of minimum-label propagation over the implicit onset-pair graph: a node rescans its slice, re-evaluates the
//                 predicate, takes the smallest label among its partners and itself, then follows label[label[..]] (pointer jumping,
//                 NS_JUMPS steps).  Reads label_in, writes label_out: a round's result does not depend on the order lanes run in.  A
//                 node whose label moved stores 1 to *changed and the round's mark to item_mark[item] (every writer stores the same
//                 value).  Labels only ever fall and stay inside the component, so the fixed point is label = smallest node of the
//                 component -- a reference whenever the component has an edge.
//   k_ns_match    one wavefront per reference v; only roots (label[v] == v) work.  The caller has sorted both sides by label, so the
//                 component's references and estimates are two runs found by binary search.  Lane l holds estimate l; per reference the
//                 64 lanes evaluate both predicates and __ballot hands back that reference's two adjacency words (onset pairs;
//                 onset-and-offset pairs) in LDS.  Lanes 0 and 1 then run Kuhn's augmenting-path search of k_mpe_match (mpe.hip) on the
//                 two graphs: explicit stack, `seen` mask per root.  A component over NS_MAX x NS_MAX stores 1 to item_flag[item].
//   k_ns_sums     one wavefront per item: n_ref, n_est, tp, tp_no_offset (int64) and the flag, summed in lane order then across lanes.
//
// The offset pairs are a subset of the onset pairs, so a component of the onset graph is a union of components of the offset graph and
// one decomposition serves both matchings.  The size of a maximum matching is unique: the order of the search cannot change a count.
#include "common.h"
#include <math.h>

#define NS_MAX 64                               // = tt_notescore_max(): references and estimates per component the matcher holds
#define NS_JUMPS 6                              // pointer-jumping steps per round
#define NS_SEARCH 32                            // binary-search steps: enough for any int32 range

static_assert(NS_MAX == 64, "one adjacency word per reference, one lane per estimate");

namespace {

typedef unsigned long long u64;

// np.around(x, 4)
__device__ __forceinline__ double ns_rnd(double x) { return rint(x * 1e4) / 1e4; }

// a NaN anywhere makes a compare false
__device__ __forceinline__ bool ns_onset_pair(double p_r, double on_r, double p_e, double on_e, double onset_tol, double pitch_tol) {
    return ns_rnd(fabs(on_r - on_e)) <= onset_tol && fabs(p_r - p_e) <= pitch_tol;
}
// np.maximum(offset_ratio * (off_r - on_r), offset_min_tolerance): a NaN operand gives NaN
__device__ __forceinline__ double ns_offset_tol(double on_r, double off_r, double ratio, double floor_tol) {
    const double t = ratio * (off_r - on_r);
    return (t != t || floor_tol != floor_tol) ? (t != t ? t : floor_tol) : (t > floor_tol ? t : floor_tol);
}
__device__ __forceinline__ bool ns_offset_pair(double off_r, double off_e, double tol_r) { return ns_rnd(fabs(off_r - off_e)) <= tol_r; }

__device__ __forceinline__ long ns_clamp(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// first index in [a, b) whose value is not below x (NaN entries, sorted last, count as +inf)
__device__ __forceinline__ long ns_lower(const double* __restrict__ v, long a, long b, double x) {
    for (int s = 0; s < NS_SEARCH; ++s) {
        if (a >= b) break;
        const long m = a + ((b - a) >> 1);
        if (v[m] < x) a = m + 1;
        else b = m;
    }
    return a;
}
// first index in [a, b) whose value is above x (NaN entries count as +inf)
__device__ __forceinline__ long ns_upper(const double* __restrict__ v, long a, long b, double x) {
    for (int s = 0; s < NS_SEARCH; ++s) {
        if (a >= b) break;
        const long m = a + ((b - a) >> 1);
        if (v[m] <= x) a = m + 1;
        else b = m;
    }
    return a;
}
// [first index with value >= x, first index with value > x) of a non-decreasing int array
__device__ __forceinline__ void ns_run(const int* __restrict__ v, long n, int x, long& lo, long& hi) {
    long a = 0, b = n;
    for (int s = 0; s < NS_SEARCH; ++s) {
        if (a >= b) break;
        const long m = a + ((b - a) >> 1);
        if (v[m] < x) a = m + 1;
        else b = m;
    }
    lo = a;
    b = n;
    for (int s = 0; s < NS_SEARCH; ++s) {
        if (a >= b) break;
        const long m = a + ((b - a) >> 1);
        if (v[m] <= x) a = m + 1;
        else b = m;
    }
    hi = a;
}

__global__ __launch_bounds__(256) void k_ns_times(const int* __restrict__ on_f, const int* __restrict__ end_f, long n, long hop_int,
                                                  double hop_mul, double denom, double* __restrict__ onset, double* __restrict__ offset) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    onset[i] = (double)((long)on_f[i] * hop_int) * hop_mul / denom;
    offset[i] = (double)((long)end_f[i] * hop_int) * hop_mul / denom;
}

__global__ __launch_bounds__(256) void k_ns_ranges(const int* __restrict__ ref_item, const double* __restrict__ ref_on, long R,
                                                   const int* __restrict__ est_item, const double* __restrict__ est_on, long E,
                                                   const long* __restrict__ ref_seg, const long* __restrict__ est_seg, int B, double window,
                                                   int* __restrict__ lo, int* __restrict__ hi) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= R + E) return;
    const bool is_ref = v < R;
    const int b = is_ref ? ref_item[v] : est_item[v - R];
    const double on = is_ref ? ref_on[v] : est_on[v - R];
    const double* __restrict__ other = is_ref ? est_on : ref_on;
    const long* __restrict__ seg = is_ref ? est_seg : ref_seg;
    const long n_other = is_ref ? E : R;
    long a = 0, z = 0;
    if (b >= 0 && b < B) {                       // an item outside [0, B) has no partners
        const long s0 = ns_clamp(seg[b], 0, n_other), s1 = ns_clamp(seg[b + 1], s0, n_other);
        a = ns_lower(other, s0, s1, on - window);
        z = ns_upper(other, a, s1, on + window);
        if (on != on) z = a;                     // a NaN onset: `on - window` compares false everywhere, nothing to scan
    }
    lo[v] = (int)a;
    hi[v] = (int)z;
}

__global__ __launch_bounds__(256) void k_ns_labels(const int* __restrict__ ref_item, const double* __restrict__ ref_p,
                                                   const double* __restrict__ ref_on, long R, const int* __restrict__ est_item,
                                                   const double* __restrict__ est_p, const double* __restrict__ est_on, long E,
                                                   const int* __restrict__ lo, const int* __restrict__ hi, double onset_tol, double pitch_tol,
                                                   const int* __restrict__ label_in, int* __restrict__ label_out, int* __restrict__ changed,
                                                   int* __restrict__ item_mark, int B, int mark) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    const long N = R + E;
    if (v >= N) return;
    const bool is_ref = v < R;
    const long self = is_ref ? v : v - R;
    const double p = is_ref ? ref_p[self] : est_p[self], on = is_ref ? ref_on[self] : est_on[self];
    const double* __restrict__ op = is_ref ? est_p : ref_p;
    const double* __restrict__ oon = is_ref ? est_on : ref_on;
    const long n_other = is_ref ? E : R, base = is_ref ? R : 0;
    const long a = ns_clamp(lo[v], 0, n_other), z = ns_clamp(hi[v], a, n_other);
    const int old = label_in[v];
    long best = ns_clamp(old, 0, N - 1);
    for (long u = a; u < z; ++u) {               // bounded by the slice the caller's tt_notescore_ranges wrote: at most n_other
        const bool pair = is_ref ? ns_onset_pair(p, on, op[u], oon[u], onset_tol, pitch_tol) : ns_onset_pair(op[u], oon[u], p, on, onset_tol, pitch_tol);
        if (pair) {
            const long l = ns_clamp(label_in[base + u], 0, N - 1);
            best = l < best ? l : best;
        }
    }
#pragma unroll
    for (int j = 0; j < NS_JUMPS; ++j) {
        const long l = ns_clamp(label_in[best], 0, N - 1);
        best = l < best ? l : best;
    }
    label_out[v] = (int)best;
    if ((int)best != old) {
        *changed = 1;
        const int b = is_ref ? ref_item[self] : est_item[self];
        if (b >= 0 && b < B) item_mark[b] = mark;
    }
}

__global__ __launch_bounds__(64) void k_ns_match(const int* __restrict__ label, const int* __restrict__ ref_lab, const int* __restrict__ ref_perm,
                                                 const int* __restrict__ est_lab, const int* __restrict__ est_perm,
                                                 const int* __restrict__ ref_item, const double* __restrict__ ref_p,
                                                 const double* __restrict__ ref_on, const double* __restrict__ ref_off, long R,
                                                 const double* __restrict__ est_p, const double* __restrict__ est_on,
                                                 const double* __restrict__ est_off, long E, double onset_tol, double pitch_tol, double ratio,
                                                 double floor_tol, int* __restrict__ tp, int* __restrict__ tp_no, int* __restrict__ item_flag,
                                                 int B) {
    __shared__ u64 adj[2][NS_MAX];
    __shared__ short match[2][NS_MAX];
    __shared__ short stk_r[2][NS_MAX], stk_e[2][NS_MAX];
    const long v = blockIdx.x;
    const int lane = threadIdx.x;
    if (label[v] != (int)v) {                    // not the smallest node of its component: the root's wave does the work
        if (lane == 0) {
            tp[v] = 0;
            tp_no[v] = 0;
        }
        return;
    }
    long r0, r1, e0, e1;
    ns_run(ref_lab, R, (int)v, r0, r1);
    ns_run(est_lab, E, (int)v, e0, e1);
    const long nr_l = r1 - r0, ne_l = e1 - e0;
    if (nr_l > NS_MAX || ne_l > NS_MAX || nr_l <= 0 || ne_l <= 0) {
        if (lane == 0) {
            tp[v] = 0;
            tp_no[v] = 0;
            if (nr_l > NS_MAX || ne_l > NS_MAX) {            // over the capacity: the item's counts come from the host
                const int b = ref_item[v];
                if (b >= 0 && b < B) item_flag[b] = 1;
            }
        }
        return;
    }
    const int nr = (int)nr_l, ne = (int)ne_l;
    const bool live = lane < ne;
    const long k = live ? ns_clamp(est_perm[e0 + lane], 0, E - 1) : 0;
    const double ep = est_p[k], eon = est_on[k], eoff = est_off[k];
    match[0][lane] = -1;
    match[1][lane] = -1;
    for (int r = 0; r < nr; ++r) {
        const long i = ns_clamp(ref_perm[r0 + r], 0, R - 1);
        const double rp = ref_p[i], ron = ref_on[i], roff = ref_off[i];
        const bool on_pair = live && ns_onset_pair(rp, ron, ep, eon, onset_tol, pitch_tol);
        const bool off_pair = on_pair && ns_offset_pair(roff, eoff, ns_offset_tol(ron, roff, ratio, floor_tol));
        const u64 w_on = __ballot(on_pair), w_off = __ballot(off_pair);
        if (lane == 0) {
            adj[0][r] = w_off;
            adj[1][r] = w_on;
        }
    }
    __syncthreads();
    if (lane >= 2) return;
    const int c = lane;                          // 0: onset-and-offset pairs, 1: onset pairs
    int count = 0;
    for (int root = 0; root < nr; ++root) {
        u64 seen = 0ull;
        int sp = 0;
        stk_r[c][0] = (short)root;
        // every step marks a new estimate in `seen` or pops: at most 2 * NS_MAX + 2 steps per root
        for (int step = 0; step < 2 * NS_MAX + 2 && sp >= 0; ++step) {
            const int r = stk_r[c][sp];
            const u64 m = adj[c][r] & ~seen;
            if (!m) {                            // r has no untried estimate left: back to its caller
                --sp;
                continue;
            }
            const int e = __ffsll((long long)m) - 1;
            seen |= 1ull << e;
            stk_e[c][sp] = (short)e;
            const int partner = match[c][e];
            if (partner < 0) {                   // a free estimate: flip the path
                for (int q = sp; q >= 0; --q) match[c][stk_e[c][q]] = stk_r[c][q];
                ++count;
                break;
            }
            if (sp + 1 < NS_MAX) stk_r[c][++sp] = (short)partner;
            else break;                          // cannot happen (distinct references on the stack); never write past it
        }
    }
    if (c == 0) tp[v] = count;
    else tp_no[v] = count;
}

__global__ __launch_bounds__(64) void k_ns_sums(const int* __restrict__ tp, const int* __restrict__ tp_no, long R, long E,
                                                const long* __restrict__ ref_seg, const long* __restrict__ est_seg,
                                                const int* __restrict__ item_flag, int B, long* __restrict__ out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const long r0 = ns_clamp(ref_seg[b], 0, R), r1 = ns_clamp(ref_seg[b + 1], r0, R);
    const long e0 = ns_clamp(est_seg[b], 0, E), e1 = ns_clamp(est_seg[b + 1], e0, E);
    long a = 0, c = 0;
    for (long i = r0 + lane; i < r1; i += 64) {
        a += tp[i];
        c += tp_no[i];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        c += __shfl_xor(c, o, 64);
    }
    if (lane == 0) {
        long* __restrict__ row = out + (long)b * 5;
        row[0] = r1 - r0;
        row[1] = e1 - e0;
        row[2] = a;
        row[3] = c;
        row[4] = item_flag[b] != 0;
    }
}

inline bool ns_sizes_ok(int64_t R, int64_t E) { return R >= 1 && E >= 1 && R + E <= 0x7fffffffLL; }
inline unsigned ns_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" int tt_notescore_max(void) { return NS_MAX; }

extern "C" int tt_notescore_times(const int* onset_frame, const int* end_frame, int64_t n, int64_t hop_int, double hop_mul, double denom,
                                  double* onset, double* offset, void* stream) {
    if (!onset_frame || !end_frame || n < 1 || n > 0x7fffffffLL || !onset || !offset) return TT_E_BADARG;
    hipLaunchKernelGGL(k_ns_times, dim3(ns_blocks(n)), dim3(256), 0, tt_stream(stream), onset_frame, end_frame, (long)n, (long)hop_int, hop_mul,
                       denom, onset, offset);
    TT_LAUNCH_CHECK();
    return 0;
}

extern "C" int tt_notescore_ranges(const int* ref_item, const double* ref_onset, int64_t n_ref, const int* est_item, const double* est_onset,
                                   int64_t n_est, const int64_t* ref_seg, const int64_t* est_seg, int n_items, double onset_tolerance,
                                   int* lo, int* hi, void* stream) {
    if (!ref_item || !ref_onset || !est_item || !est_onset || !ns_sizes_ok(n_ref, n_est) || !ref_seg || !est_seg || n_items < 1 || !lo || !hi)
        return TT_E_BADARG;
    hipLaunchKernelGGL(k_ns_ranges, dim3(ns_blocks(n_ref + n_est)), dim3(256), 0, tt_stream(stream), ref_item, ref_onset, (long)n_ref, est_item,
                       est_onset, (long)n_est, reinterpret_cast<const long*>(ref_seg), reinterpret_cast<const long*>(est_seg), n_items,
                       onset_tolerance + 1e-4, lo, hi);
    TT_LAUNCH_CHECK();
    return 0;
}

extern "C" int tt_notescore_labels(const int* ref_item, const double* ref_pitch, const double* ref_onset, int64_t n_ref, const int* est_item,
                                   const double* est_pitch, const double* est_onset, int64_t n_est, const int* lo, const int* hi,
                                   double onset_tolerance, double pitch_tolerance, const int* label_in, int* label_out, int* changed,
                                   int* item_mark, int n_items, int mark, void* stream) {
    if (!ref_item || !ref_pitch || !ref_onset || !est_item || !est_pitch || !est_onset || !ns_sizes_ok(n_ref, n_est) || !lo || !hi || !label_in ||
        !label_out || label_in == label_out || !changed || !item_mark || n_items < 1)
        return TT_E_BADARG;
    hipLaunchKernelGGL(k_ns_labels, dim3(ns_blocks(n_ref + n_est)), dim3(256), 0, tt_stream(stream), ref_item, ref_pitch, ref_onset, (long)n_ref,
                       est_item, est_pitch, est_onset, (long)n_est, lo, hi, onset_tolerance, pitch_tolerance, label_in, label_out, changed,
                       item_mark, n_items, mark);
    TT_LAUNCH_CHECK();
    return 0;
}

extern "C" int tt_notescore_match(const int* label, const int* ref_label_sorted, const int* ref_perm, const int* est_label_sorted,
                                  const int* est_perm, const int* ref_item, const double* ref_pitch, const double* ref_onset,
                                  const double* ref_offset, int64_t n_ref, const double* est_pitch, const double* est_onset,
                                  const double* est_offset, int64_t n_est, double onset_tolerance, double pitch_tolerance, double offset_ratio,
                                  double offset_min_tolerance, int* tp, int* tp_no_offset, int* item_flag, int n_items, void* stream) {
    if (!label || !ref_label_sorted || !ref_perm || !est_label_sorted || !est_perm || !ref_item || !ref_pitch || !ref_onset || !ref_offset ||
        !est_pitch || !est_onset || !est_offset || !ns_sizes_ok(n_ref, n_est) || !tp || !tp_no_offset || !item_flag || n_items < 1)
        return TT_E_BADARG;
    hipLaunchKernelGGL(k_ns_match, dim3((unsigned)n_ref), dim3(64), 0, tt_stream(stream), label, ref_label_sorted, ref_perm, est_label_sorted,
                       est_perm, ref_item, ref_pitch, ref_onset, ref_offset, (long)n_ref, est_pitch, est_onset, est_offset, (long)n_est,
                       onset_tolerance, pitch_tolerance, offset_ratio, offset_min_tolerance, tp, tp_no_offset, item_flag, n_items);
    TT_LAUNCH_CHECK();
    return 0;
}

extern "C" int tt_notescore_sums(const int* tp, const int* tp_no_offset, int64_t n_ref, int64_t n_est, const int64_t* ref_seg,
                                 const int64_t* est_seg, const int* item_flag, int n_items, int64_t* out, void* stream) {
    if (!tp || !tp_no_offset || !ns_sizes_ok(n_ref, n_est) || !ref_seg || !est_seg || !item_flag || n_items < 1 || !out) return TT_E_BADARG;
    hipLaunchKernelGGL(k_ns_sums, dim3((unsigned)n_items), dim3(64), 0, tt_stream(stream), tp, tp_no_offset, (long)n_ref, (long)n_est,
                       reinterpret_cast<const long*>(ref_seg), reinterpret_cast<const long*>(est_seg), item_flag, n_items, out);
    TT_LAUNCH_CHECK();
    return 0;
}
