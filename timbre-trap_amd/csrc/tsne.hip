// Exact t-SNE in two dimensions on the device (include/ttrap.h: tt_tsne_*): the O(N^2) gradient of scikit-learn's method='exact' in
// float64, without atomics, every sum in an order that depends on N alone.  The semantics are stated in the header; this file is their
// only device form and tests/tsne_ref.py their NumPy restatement.
//
//   x (N, D) fp32 / fp64 --k_tsne_dist--> squared distances in P's buffer --k_tsne_search--> beta, s (one wavefront per row)
//                        --k_tsne_sym--> C + C^T in place, row sums --k_tsne_total--> the total --k_tsne_norm--> P
//   per iteration:  P, Y --k_tsne_pairs--> partial sums per (j split, row) --k_tsne_rows--> sums per row, partial Z per 256 rows
//                        --k_tsne_update--> gains, U, Y
//   after the last:  k_tsne_pairs, k_tsne_rows at the final Y, --k_tsne_klpairs--> partial KL per (j split, row) --k_tsne_final-->
//                    kl_out, gnorm_out
//
// k_tsne_pairs / k_tsne_klpairs: a workgroup owns 64 rows (lane = row i) and one of S = ts_split(N) ranges of j; its four wavefronts walk
// the range with stride four, each j in ascending order, reading P[j N + i] -- P is symmetric, so the 64 lanes read 64 adjacent doubles --
// and y_j from the range's tile of Y in LDS (one address per wavefront: a broadcast).  The four wavefronts' sums are added in wavefront
// order, the S ranges in ascending order (k_tsne_rows), 256 rows by a fixed tree, the groups of 256 rows in ascending order: nothing
// depends on the launch geometry beyond N.
//
// Every offset into P is 64-bit.  A lane whose row lies beyond N computes on row N - 1 and stores nothing.
#include "common.h"
#include <float.h>
#include <math.h>

// The restatement forms the squared distances, the entropy and the update with individually rounded operations; the divide, exp and log
// are the library's.  Nothing here may be contracted, and the file is built without fast-math flags.
#pragma clang fp contract(off)

#define TS_MIN_N 2
#define TS_MAX_N 16384                          // P stays within 2 GiB
#define TS_STEPS 128                            // evaluations of the perplexity search: no tolerance exit (see the header)
#define TS_ROWS 64                              // rows per workgroup of the pair kernels
#define TS_WAVES 4                              // wavefronts per workgroup of the pair kernels
#define TS_MAX_SPLIT 64                         // ranges of j at most; with TS_MAX_N: 256 j per range at most
#define TS_TILE 256                             // j per range at most = the tile of Y in LDS
#define TS_GROUP 256                            // rows per workgroup of k_tsne_rows / k_tsne_update
#define TS_MAX_GROUPS (TS_MAX_N / TS_GROUP)

namespace {

inline int ts_split(int N) {
    const int s = (N + TS_ROWS - 1) / TS_ROWS;
    return s > TS_MAX_SPLIT ? TS_MAX_SPLIT : s;
}
inline int ts_chunk(int N) { return (N + ts_split(N) - 1) / ts_split(N); }
inline int ts_groups(int N) { return (N + TS_GROUP - 1) / TS_GROUP; }

// scratch, in doubles: part [5][S][N] (k_tsne_klpairs reuses its first plane) | rowacc [5][N] | zpart [TS_MAX_GROUPS] | s [N] | rowsum [N]
// | total [1]
struct TsScratch {
    double *part, *rowacc, *zpart, *s, *rowsum, *total;
};
inline int64_t ts_scratch_doubles(int N) { return (int64_t)5 * ts_split(N) * N + (int64_t)5 * N + TS_MAX_GROUPS + 2 * (int64_t)N + 8; }
inline TsScratch ts_carve(void* scratch, int N) {
    TsScratch c;
    c.part = static_cast<double*>(scratch);
    c.rowacc = c.part + (int64_t)5 * ts_split(N) * N;
    c.zpart = c.rowacc + (int64_t)5 * N;
    c.s = c.zpart + TS_MAX_GROUPS;
    c.rowsum = c.s + N;
    c.total = c.rowsum + N;
    return c;
}

// sum of v[0 .. n) by the 256 threads of a workgroup: thread t adds v[t], v[t + 256], ... in ascending order, then a fixed tree
__device__ __forceinline__ double ts_block_sum(const double* __restrict__ v, int n, double* sh) {
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) a += v[i];
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    return sh[0];
}

// ---- affinities -----------------------------------------------------------------------------------------------------------------------

// D[i][j] = sum over d ascending of (x[i][d] - x[j][d])^2; 16 x 16 outputs per workgroup, 16 dimensions per tile.  Dimensions beyond D
// read as 0 on both sides and add +0, which changes no bit.
template <typename T>
__global__ __launch_bounds__(256) void k_tsne_dist(const T* __restrict__ x, int N, int D, double* __restrict__ out) {
    __shared__ double sa[16][17], sb[16][17];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int i = blockIdx.y * 16 + ty, j = blockIdx.x * 16 + tx;
    const int ra = blockIdx.y * 16 + ty, rb = blockIdx.x * 16 + ty;          // the rows this thread stages
    double acc = 0.0;
    for (int d0 = 0; d0 < D; d0 += 16) {
        const int d = d0 + tx;
        sa[ty][tx] = ra < N && d < D ? (double)x[(long)ra * D + d] : 0.0;
        sb[ty][tx] = rb < N && d < D ? (double)x[(long)rb * D + d] : 0.0;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const double t = sa[ty][k] - sb[tx][k];
            acc += t * t;
        }
        __syncthreads();
    }
    if (i < N && j < N) out[(long)i * N + j] = acc;
}

// One wavefront per row: TS_STEPS evaluations of scikit-learn's search for beta (start at 1, double or halve until bracketed, then
// midpoints).  The two sums of an evaluation: lane l adds j = l, l + 64, ... in ascending order, then the xor butterfly, which leaves
// the same bits in every lane, so the whole wavefront takes the same branch.
__global__ __launch_bounds__(256) void k_tsne_search(const double* __restrict__ dist, int N, double target, double* __restrict__ beta_out,
                                                     double* __restrict__ s_out) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    const double* __restrict__ row = dist + (long)i * N;
    double beta = 1.0, lo = -INFINITY, hi = INFINITY, se = 0.0;
    for (int step = 0;; ++step) {
        double sd = 0.0;
        se = 0.0;
        for (int j = lane; j < N; j += 64) {
            if (j == i) continue;
            const double d = row[j];
            const double e = exp(-(d * beta));
            se += e;
            sd += d * e;
        }
        se = wave_sum_d(se);
        sd = wave_sum_d(sd);
        if (se == 0.0) se = 1e-8;
        if (step == TS_STEPS - 1) break;
        const double h = log(se) + beta * (sd / se);
        if (h - target > 0.0) {
            lo = beta;
            beta = hi == INFINITY ? beta * 2.0 : (beta + hi) / 2.0;
        } else {
            hi = beta;
            beta = lo == -INFINITY ? beta / 2.0 : (beta + lo) / 2.0;
        }
    }
    if (lane == 0) {
        beta_out[i] = beta;
        s_out[i] = se;
    }
}

// In place, one wavefront per row: distance -> C[i][j] + C[j][i], C[i][j] = exp(-beta_i d) / s_i; the same two terms in either triangle, and
// the addition commutes, so the result is symmetric bit for bit.  rowsum[i]: lane partial sums, then the butterfly.
__global__ __launch_bounds__(256) void k_tsne_sym(double* __restrict__ P, int N, const double* __restrict__ beta, const double* __restrict__ s,
                                                  double* __restrict__ rowsum) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    double* __restrict__ row = P + (long)i * N;
    const double bi = beta[i], si = s[i];
    double acc = 0.0;
    for (int j = lane; j < N; j += 64) {
        double v = 0.0;
        if (j != i) {
            const double d = row[j];
            v = exp(-(d * bi)) / si + exp(-(d * beta[j])) / s[j];
        }
        row[j] = v;
        acc += v;
    }
    acc = wave_sum_d(acc);
    if (lane == 0) rowsum[i] = acc;
}

__global__ __launch_bounds__(256) void k_tsne_total(const double* __restrict__ rowsum, int N, double* __restrict__ total) {
    __shared__ double sh[256];
    const double t = ts_block_sum(rowsum, N, sh);
    if (threadIdx.x == 0) total[0] = t > DBL_EPSILON ? t : DBL_EPSILON;
}

__global__ __launch_bounds__(256) void k_tsne_norm(double* __restrict__ P, int N, const double* __restrict__ total) {
    const int i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    const double t = total[0];
    double* p = P + (long)i * N + j;
    const double v = *p / t;
    *p = i == j ? 0.0 : (v > DBL_EPSILON ? v : DBL_EPSILON);
}

// ---- iterations -----------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ double ts_z(const double* __restrict__ zpart, int groups) {
    double z = 0.0;
    for (int g = 0; g < groups; ++g) z += zpart[g];
    return z;
}

// stage the tile of Y for the workgroup's range of j; returns the range
__device__ __forceinline__ void ts_stage(const double* __restrict__ Y, int N, int chunk, double (*sY)[2], int& j0, int& j1) {
    j0 = blockIdx.y * chunk;
    j0 = j0 > N ? N : j0;
    j1 = j0 + chunk > N ? N : j0 + chunk;
    for (int k = threadIdx.x; k < j1 - j0; k += 64 * TS_WAVES) {
        sY[k][0] = Y[2 * (long)(j0 + k)];
        sY[k][1] = Y[2 * (long)(j0 + k) + 1];
    }
    __syncthreads();
}

// part[q][s][i], q = 0, 1: sum_j p w (y_i - y_j); q = 2, 3: sum_j w^2 (y_i - y_j); q = 4: sum_{j != i} w; over the j of range s
__global__ __launch_bounds__(64 * TS_WAVES) void k_tsne_pairs(const double* __restrict__ P, const double* __restrict__ Y, int N, int chunk,
                                                              double* __restrict__ part) {
    __shared__ double sY[TS_TILE][2];
    __shared__ double sAcc[TS_WAVES][5][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int j0, j1;
    ts_stage(Y, N, chunk, sY, j0, j1);
    const int i = blockIdx.x * TS_ROWS + lane;
    const int ic = i < N ? i : N - 1;
    const double y0 = Y[2 * (long)ic], y1 = Y[2 * (long)ic + 1];
    const double* __restrict__ Pc = P + ic;
    double a0 = 0.0, a1 = 0.0, r0 = 0.0, r1 = 0.0, sw = 0.0;
#pragma unroll 4
    for (int j = j0 + wave; j < j1; j += TS_WAVES) {
        const double p = Pc[(long)j * N];
        const double d0 = y0 - sY[j - j0][0], d1 = y1 - sY[j - j0][1];
        const double w = 1.0 / (1.0 + (d0 * d0 + d1 * d1));
        const double pw = p * w, ww = w * w;
        a0 += pw * d0;
        a1 += pw * d1;
        r0 += ww * d0;
        r1 += ww * d1;
        sw += j == ic ? 0.0 : w;
    }
    sAcc[wave][0][lane] = a0;
    sAcc[wave][1][lane] = a1;
    sAcc[wave][2][lane] = r0;
    sAcc[wave][3][lane] = r1;
    sAcc[wave][4][lane] = sw;
    __syncthreads();
    if (wave == 0 && i < N) {
        const long S = gridDim.y;
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            double v = sAcc[0][q][lane];
#pragma unroll
            for (int w = 1; w < TS_WAVES; ++w) v += sAcc[w][q][lane];
            part[(q * S + blockIdx.y) * N + i] = v;
        }
    }
}

// rowacc[q][i] = the S ranges of part added in ascending order; zpart[group] = sum of rowacc[4] over the group's 256 rows (fixed tree)
__global__ __launch_bounds__(TS_GROUP) void k_tsne_rows(const double* __restrict__ part, int N, int S, double* __restrict__ rowacc,
                                                        double* __restrict__ zpart) {
    __shared__ double sh[TS_GROUP];
    const int i = blockIdx.x * TS_GROUP + threadIdx.x;
    double sw = 0.0;
    if (i < N) {
        for (int q = 0; q < 5; ++q) {
            double v = 0.0;
            for (long s = 0; s < S; ++s) v += part[(q * (long)S + s) * N + i];
            rowacc[(long)q * N + i] = v;
            if (q == 4) sw = v;
        }
    }
    sh[threadIdx.x] = sw;
    __syncthreads();
    for (int o = TS_GROUP / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) zpart[blockIdx.x] = sh[0];
}

__device__ __forceinline__ double ts_grad(const double* __restrict__ rowacc, int N, int i, int k, double e, double z) {
    return 4.0 * (e * rowacc[(long)k * N + i] - rowacc[(long)(2 + k) * N + i] / z);
}

// scikit-learn's _gradient_descent, one thread per row
__global__ __launch_bounds__(TS_GROUP) void k_tsne_update(const double* __restrict__ rowacc, const double* __restrict__ zpart, int N, int groups,
                                                          double e, double momentum, double lr, double min_gain, double* __restrict__ Y,
                                                          double* __restrict__ U, double* __restrict__ gains) {
    const int i = blockIdx.x * TS_GROUP + threadIdx.x;
    if (i >= N) return;
    const double z = ts_z(zpart, groups);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double g = ts_grad(rowacc, N, i, k, e, z);
        const long o = 2 * (long)i + k;
        double u = U[o], gn = gains[o];
        gn = u * g < 0.0 ? gn + 0.2 : gn * 0.8;
        gn = gn < min_gain ? min_gain : gn;
        u = momentum * u - lr * (g * gn);
        gains[o] = gn;
        U[o] = u;
        Y[o] += u;
    }
}

// klpart[s][i] = sum over the j != i of range s of p log(max(p, eps) / max(w / Z, eps))
__global__ __launch_bounds__(64 * TS_WAVES) void k_tsne_klpairs(const double* __restrict__ P, const double* __restrict__ Y,
                                                                const double* __restrict__ zpart, int N, int chunk, int groups,
                                                                double* __restrict__ klpart) {
    __shared__ double sY[TS_TILE][2];
    __shared__ double sAcc[TS_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int j0, j1;
    ts_stage(Y, N, chunk, sY, j0, j1);
    const double z = ts_z(zpart, groups);
    const int i = blockIdx.x * TS_ROWS + lane;
    const int ic = i < N ? i : N - 1;
    const double y0 = Y[2 * (long)ic], y1 = Y[2 * (long)ic + 1];
    const double* __restrict__ Pc = P + ic;
    double kl = 0.0;
    for (int j = j0 + wave; j < j1; j += TS_WAVES) {
        if (j == ic) continue;
        double p = Pc[(long)j * N];
        const double d0 = y0 - sY[j - j0][0], d1 = y1 - sY[j - j0][1];
        const double w = 1.0 / (1.0 + (d0 * d0 + d1 * d1));
        double q = w / z;
        q = q > DBL_EPSILON ? q : DBL_EPSILON;
        const double pc = p > DBL_EPSILON ? p : DBL_EPSILON;
        kl += p * log(pc / q);
    }
    sAcc[wave][lane] = kl;
    __syncthreads();
    if (wave == 0 && i < N) {
        double v = sAcc[0][lane];
#pragma unroll
        for (int w = 1; w < TS_WAVES; ++w) v += sAcc[w][lane];
        klpart[(long)blockIdx.y * N + i] = v;
    }
}

// one workgroup: KL = the rows' sums (ranges ascending) added by ts_block_sum's order; the norm of the unexaggerated gradient at Y
__global__ __launch_bounds__(256) void k_tsne_final(const double* __restrict__ klpart, const double* __restrict__ rowacc,
                                                    const double* __restrict__ zpart, int N, int S, int groups, double* __restrict__ kl_out,
                                                    double* __restrict__ gnorm_out) {
    __shared__ double sh[256];
    const double z = ts_z(zpart, groups);
    double kl = 0.0, gg = 0.0;
    for (int i = threadIdx.x; i < N; i += 256) {
        double v = 0.0;
        for (long s = 0; s < S; ++s) v += klpart[s * N + i];
        kl += v;
        const double g0 = ts_grad(rowacc, N, i, 0, 1.0, z), g1 = ts_grad(rowacc, N, i, 1, 1.0, z);
        gg += g0 * g0;
        gg += g1 * g1;
    }
    for (int pass = 0; pass < 2; ++pass) {
        sh[threadIdx.x] = pass ? gg : kl;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            if (pass) gnorm_out[0] = sqrt(sh[0]);
            else kl_out[0] = sh[0];
        }
        __syncthreads();
    }
}

inline bool ts_n_ok(int N) { return N >= TS_MIN_N && N <= TS_MAX_N; }
inline bool ts_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

int ts_launch_pairs(const double* P, const double* Y, int N, const TsScratch& c, hipStream_t st) {
    const int S = ts_split(N);
    hipLaunchKernelGGL(k_tsne_pairs, dim3((N + TS_ROWS - 1) / TS_ROWS, S), dim3(64 * TS_WAVES), 0, st, P, Y, N, ts_chunk(N), c.part);
    TT_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_tsne_rows, dim3(ts_groups(N)), dim3(TS_GROUP), 0, st, c.part, N, S, c.rowacc, c.zpart);
    TT_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int64_t tt_tsne_scratch_bytes(int N) { return ts_n_ok(N) ? ts_scratch_doubles(N) * 8 : (int64_t)TT_E_BADARG; }

extern "C" int tt_tsne_affinities(const void* x, int dtype, int N, int D, double perplexity, double* P, double* beta, void* scratch,
                                  void* stream) {
    if (!x || (dtype != 0 && dtype != 1) || !ts_n_ok(N) || D < 1 || !(perplexity > 0.0 && perplexity < (double)N) || !P || !beta ||
        !scratch || !ts_aligned(P) || !ts_aligned(beta) || !ts_aligned(scratch))
        return TT_E_BADARG;
    const TsScratch c = ts_carve(scratch, N);
    hipStream_t st = tt_stream(stream);
    const dim3 tiles((N + 15) / 16, (N + 15) / 16);
    if (dtype == 0) hipLaunchKernelGGL(k_tsne_dist<float>, tiles, dim3(256), 0, st, static_cast<const float*>(x), N, D, P);
    else hipLaunchKernelGGL(k_tsne_dist<double>, tiles, dim3(256), 0, st, static_cast<const double*>(x), N, D, P);
    TT_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_tsne_search, dim3((N + 3) / 4), dim3(256), 0, st, P, N, log(perplexity), beta, c.s);
    TT_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_tsne_sym, dim3((N + 3) / 4), dim3(256), 0, st, P, N, beta, c.s, c.rowsum);
    TT_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_tsne_total, dim3(1), dim3(256), 0, st, c.rowsum, N, c.total);
    TT_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_tsne_norm, dim3((N + 255) / 256, N), dim3(256), 0, st, P, N, c.total);
    TT_LAUNCH_CHECK();
    return 0;
}

extern "C" int tt_tsne_run(const double* P, int N, double* Y, double* U, double* gains, int it0, int it1, int explore_iters,
                           double exaggeration, double learning_rate, double momentum0, double momentum1, double min_gain, double* kl_out,
                           double* gnorm_out, void* scratch, void* stream) {
    if (!P || !ts_n_ok(N) || !Y || !U || !gains || it0 < 0 || it1 < it0 || explore_iters < 0 || !(exaggeration > 0.0) ||
        !(learning_rate > 0.0) || !(momentum0 >= 0.0 && momentum0 < 1.0) || !(momentum1 >= 0.0 && momentum1 < 1.0) || !(min_gain >= 0.0) ||
        !kl_out || !gnorm_out || !scratch || !ts_aligned(P) || !ts_aligned(Y) || !ts_aligned(U) || !ts_aligned(gains) ||
        !ts_aligned(kl_out) || !ts_aligned(gnorm_out) || !ts_aligned(scratch))
        return TT_E_BADARG;
    const TsScratch c = ts_carve(scratch, N);
    hipStream_t st = tt_stream(stream);
    const int S = ts_split(N), groups = ts_groups(N);
    for (int it = it0; it < it1; ++it) {
        const bool explore = it < explore_iters;
        if (int rc = ts_launch_pairs(P, Y, N, c, st)) return rc;
        hipLaunchKernelGGL(k_tsne_update, dim3(groups), dim3(TS_GROUP), 0, st, c.rowacc, c.zpart, N, groups, explore ? exaggeration : 1.0,
                           explore ? momentum0 : momentum1, learning_rate, min_gain, Y, U, gains);
        TT_LAUNCH_CHECK();
    }
    if (int rc = ts_launch_pairs(P, Y, N, c, st)) return rc;
    hipLaunchKernelGGL(k_tsne_klpairs, dim3((N + TS_ROWS - 1) / TS_ROWS, S), dim3(64 * TS_WAVES), 0, st, P, Y, c.zpart, N, ts_chunk(N), groups,
                       c.part);
    TT_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_tsne_final, dim3(1), dim3(256), 0, st, c.part, c.rowacc, c.zpart, N, S, groups, kl_out, gnorm_out);
    TT_LAUNCH_CHECK();
    return 0;
}
