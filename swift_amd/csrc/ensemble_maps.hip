// Per-grid-point verification terms of an ensemble against the verifying fields (swiftk_ensemble_maps, include/swiftk.h): bias,
// squared error, fair CRPS and member variance of every pixel, written or added into a resident fp64 buffer -- the maps of
// `swift_amd.generate --maps`, accumulated over initial conditions.  All arithmetic in fp64 in one documented order per pixel,
// so one set of bits serves every batch shape.
#include "common.h"

#include <math.h>

// Rounded fp64 operations that stay separate (ensemble_summary.hip: the plain operators, and hipcc's __dadd_rn family, are
// contracted into FMAs; these are not).  A quotient has nothing to fuse with, and |.| is exact.
static __device__ __forceinline__ double dadd_rn(double x, double y) { return __ocml_add_rte_f64(x, y); }
static __device__ __forceinline__ double dsub_rn(double x, double y) { return __ocml_sub_rte_f64(x, y); }
static __device__ __forceinline__ double dmul_rn(double x, double y) { return __ocml_mul_rte_f64(x, y); }

// The four terms of one pixel from its members x[0 .. N) (M - 4 < N <= M, N the same in every lane: no lane diverges at the
// `live` tests, and all but those of the last three members are decided at compile time) and its truth y.
//   bias      s = sum x_m in member order; mean = s / N; e = mean - y
//   mse       e e
//   crps      a = sum_m |x_m - y|; p = sum_{m < m'} |x_m - x_m'|, m outside, m' inside, both ascending; a / N - p / (N (N - 1))
//   variance  v = sum_m (x_m - mean)^2, difference, product and sum rounded separately; v / (N - 1)
// Equal members: every |x_m - x_m'| and every x_m - mean is +0 (N x is exact for N <= 64), so p and v are exactly 0.
template <int M>
static __device__ __forceinline__ void pixel_terms(const float (&xf)[M], float yf, int N, double (&t)[4]) {
#define SWIFTK_MAPS_LIVE(m) ((m) <= M - 4 || (m) < N)
    const double y = (double)yf, dn = (double)N, dn1 = (double)(N - 1), dnn = (double)(N * (N - 1));
    double x[M];
#pragma unroll
    for (int m = 0; m < M; ++m) x[m] = (double)xf[m];
    double s = 0.0, a = 0.0;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        if (SWIFTK_MAPS_LIVE(m)) {
            s = dadd_rn(s, x[m]);
            a = dadd_rn(a, fabs(dsub_rn(x[m], y)));
        }
    }
    const double mean = __ddiv_rn(s, dn), e = dsub_rn(mean, y);
    double v = 0.0, p = 0.0;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        if (SWIFTK_MAPS_LIVE(m)) {
            const double d = dsub_rn(x[m], mean);
            v = dadd_rn(v, dmul_rn(d, d));
        }
    }
#pragma unroll
    for (int m = 0; m < M - 1; ++m) {
        if (SWIFTK_MAPS_LIVE(m)) {
#pragma unroll
            for (int k = m + 1; k < M; ++k)
                if (SWIFTK_MAPS_LIVE(k)) p = dadd_rn(p, fabs(dsub_rn(x[m], x[k])));
        }
    }
    t[0] = e;
    t[1] = dmul_rn(e, e);
    t[2] = dsub_rn(__ddiv_rn(a, dn), __ddiv_rn(p, dnn));
    t[3] = __ddiv_rn(v, dn1);
#undef SWIFTK_MAPS_LIVE
}

// A thread owns PX pixels of an (i, v) plane, 256 apart (every load and store coalesced along w): blockIdx.x walks the planes,
// blockIdx.y and the threads the plane's H W pixels, both in strides of the grid.  It issues the PX (N + 1) loads of its pixels
// (members V H W floats apart) -- and, when accumulating, the 4 PX loads of acc -- before it uses any: the kernel streams, and like
// rank_hist.hip it lives on the loads in flight, so small ensembles take more pixels per thread (PX M = 16 up to 8 members, one
// pixel of M members beyond).  One kernel per multiple of 4 members, the column in registers, the rest of x never read.
// A pixel past the plane's end is read as its last pixel and not stored: the loads stay unconditional and in bounds.
//
// acc[i, s, v, h, w] = accumulate ? acc + term_s : term_s, one rounded add: every element is written by exactly one thread, with
// accumulate == 0 without being read -- no atomics, no scratch, no clearing.
template <int M, int PX>
__global__ __launch_bounds__(256) static void ensemble_maps_kernel(const float* __restrict__ pred, const float* __restrict__ y,
                                                                   double* __restrict__ acc, int N, int V, int H, int W,
                                                                   int accumulate, int64_t planes) {
    const int64_t hw = (int64_t)H * W, sstride = (int64_t)V * hw;  // members, and statistics, lie V H W elements apart
    for (int64_t plane = blockIdx.x; plane < planes; plane += gridDim.x) {
        const int64_t i = plane / V, v = plane - i * V;
        const float* xp = pred + (i * N * V + v) * hw;
        const float* yp = y + plane * hw;
        double* ap = acc + (i * 4 * V + v) * hw;
        for (int64_t at0 = (int64_t)blockIdx.y * (256 * PX) + threadIdx.x; at0 < hw; at0 += (int64_t)gridDim.y * (256 * PX)) {
            int64_t at[PX];
            float x[PX][M], yv[PX];
            double old[PX][4] = {};
#pragma unroll
            for (int k = 0; k < PX; ++k) {
                at[k] = at0 + k * 256 < hw ? at0 + k * 256 : hw - 1;
                yv[k] = yp[at[k]];
#pragma unroll
                for (int m = 0; m < M; ++m) x[k][m] = (m <= M - 4 || m < N) ? xp[at[k] + m * sstride] : 0.0f;
            }
            if (accumulate) {
#pragma unroll
                for (int k = 0; k < PX; ++k)
#pragma unroll
                    for (int s = 0; s < 4; ++s) old[k][s] = ap[at[k] + s * sstride];
            }
#pragma unroll
            for (int k = 0; k < PX; ++k) {
                double t[4];
                pixel_terms<M>(x[k], yv[k], N, t);
                if (at0 + k * 256 < hw) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) ap[at[k] + s * sstride] = accumulate ? dadd_rn(old[k][s], t[s]) : t[s];
                }
            }
        }
    }
}

extern "C" int swiftk_ensemble_maps(const float* pred, const float* y, double* acc, int n, int N, int V, int H, int W,
                                    int accumulate, void* stream) {
    if (!pred || !y || !acc || n <= 0 || N <= 0 || V <= 0 || H <= 0 || W <= 0) return SWIFTK_EINVAL;
    if (accumulate != 0 && accumulate != 1) return SWIFTK_EINVAL;
    if (N < 2 || N > 64 || (int64_t)n * V > INT32_MAX) return SWIFTK_ESHAPE;
    if ((((uintptr_t)pred | (uintptr_t)y) & 3) || ((uintptr_t)acc & 7)) return SWIFTK_EALIGN;
    const int M = (N + 3) & ~3, px = M <= 4 ? 4 : M <= 8 ? 2 : 1;
    const int64_t planes = (int64_t)n * V, hw = (int64_t)H * W, chunks = (hw + 256 * px - 1) / (256 * px);
    // the grid strides over planes and pixels beyond these caps (1M planes x 4096 blocks of a plane)
    const dim3 grid((unsigned)(planes < (1 << 20) ? planes : (1 << 20)), (unsigned)(chunks < 4096 ? chunks : 4096));
    hipStream_t s = static_cast<hipStream_t>(stream);
#define SWIFTK_MAPS_LAUNCH(M_, PX_)                                                                                          \
    case M_:                                                                                                                 \
        hipLaunchKernelGGL((ensemble_maps_kernel<M_, PX_>), grid, dim3(256), 0, s, pred, y, acc, N, V, H, W, accumulate, \
                           planes);                                                                                          \
        break;
    switch (M) {  // the members padded to a multiple of 4
        SWIFTK_MAPS_LAUNCH(4, 4)
        SWIFTK_MAPS_LAUNCH(8, 2)
        SWIFTK_MAPS_LAUNCH(12, 1)
        SWIFTK_MAPS_LAUNCH(16, 1)
        SWIFTK_MAPS_LAUNCH(20, 1)
        SWIFTK_MAPS_LAUNCH(24, 1)
        SWIFTK_MAPS_LAUNCH(28, 1)
        SWIFTK_MAPS_LAUNCH(32, 1)
        SWIFTK_MAPS_LAUNCH(36, 1)
        SWIFTK_MAPS_LAUNCH(40, 1)
        SWIFTK_MAPS_LAUNCH(44, 1)
        SWIFTK_MAPS_LAUNCH(48, 1)
        SWIFTK_MAPS_LAUNCH(52, 1)
        SWIFTK_MAPS_LAUNCH(56, 1)
        SWIFTK_MAPS_LAUNCH(60, 1)
        SWIFTK_MAPS_LAUNCH(64, 1)
    }
#undef SWIFTK_MAPS_LAUNCH
    SWIFTK_CHECK_LAUNCH();
    return 0;
}
