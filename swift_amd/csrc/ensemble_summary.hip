// Per-pixel summary of an ensemble (swiftk_ensemble_summary, include/swiftk.h): mean, spread and a table of quantiles over the
// members, the product of `swift_amd.generate --summary`.  Mean and spread in fp64 in member order, quantiles as selections from
// the sorted members plus one fp64 interpolation: one order of arithmetic per pixel serves every batch shape.
#include "common.h"

#include <math.h>

#include <utility>

// Rounded fp64 operations that stay separate.  hipcc's __dadd_rn / __dsub_rn / __dmul_rn are the plain operators unless
// OCML_BASIC_ROUNDED_OPERATIONS is defined for the whole build, and a plain product under a plain sum is fused (seen here:
// a + g (b - a) came out as one v_fmac_f64, a different number than the definition's).  These are the functions those names
// stand for under that define: round-to-nearest-even, never contracted.  A quotient and a square root have nothing to fuse with.
static __device__ __forceinline__ double dadd_rn(double x, double y) { return __ocml_add_rte_f64(x, y); }
static __device__ __forceinline__ double dsub_rn(double x, double y) { return __ocml_sub_rte_f64(x, y); }
static __device__ __forceinline__ double dmul_rn(double x, double y) { return __ocml_mul_rte_f64(x, y); }

// Element `idx` (0 <= idx < M, the same in every lane) of a register array by a binary tree of selects, one level per bit of
// idx: M - 1 selects at most, every index a compile-time one, so the array never leaves the registers.  (An odd level's last
// element has no partner; idx < M never asks for it.)
template <int M>
static __device__ __forceinline__ float pick(const float (&x)[M], int idx) {
    float t[M];
#pragma unroll
    for (int k = 0; k < M; ++k) t[k] = x[k];
#pragma unroll
    for (int w = M, bit = 0; w > 1; w = (w + 1) / 2, ++bit) {
        const bool odd = (idx >> bit) & 1;
#pragma unroll
        for (int k = 0; k < (w + 1) / 2; ++k) t[k] = 2 * k + 1 < w ? (odd ? t[2 * k + 1] : t[2 * k]) : t[2 * k];
    }
    return t[0];
}

// Batcher's odd-even merge sort of P = 2^k inputs, as a list of compare-exchanges (a < b, the smaller value to a), cut down to
// M <= P inputs: every exchange moves the larger value up, so inputs M .. P - 1 held at +inf would never move, and every exchange
// that touches one is dropped.  What is left sorts M inputs (42 exchanges at 12 where the full 16 take 63; 543 at 64).
struct SortNet {
    int n;
    unsigned char a[544], b[544];
};
template <int P, int M>
constexpr SortNet make_sort_net() {
    SortNet r{};
    for (int p = 1; p < P; p <<= 1)
        for (int k = p; k >= 1; k >>= 1)
            for (int j = k % p; j + k < P; j += 2 * k)
                for (int i = 0; i < k && i + j + k < P; ++i)
                    if ((i + j) / (2 * p) == (i + j + k) / (2 * p) && i + j + k < M) {
                        r.a[r.n] = (unsigned char)(i + j);
                        r.b[r.n] = (unsigned char)(i + j + k);
                        ++r.n;
                    }
    return r;
}
template <int P, int M>
inline constexpr SortNet kSortNet = make_sort_net<P, M>();
template <int A, int B, int M>
static __device__ __forceinline__ void exchange(float (&x)[M]) {
    const float lo = fminf(x[A], x[B]), hi = fmaxf(x[A], x[B]);
    x[A] = lo;
    x[B] = hi;
}
// (the indices as template arguments: constants by construction, and the table itself is never emitted)
template <int P, int M, int... Is>
static __device__ __forceinline__ void sort_ascending(float (&x)[M], std::integer_sequence<int, Is...>) {
    (exchange<kSortNet<P, M>.a[Is], kSortNet<P, M>.b[Is]>(x), ...);
}

// A thread owns a pixel of an (i, v) plane: blockIdx.x walks the planes, blockIdx.y and the threads the plane's H W pixels
// (coalesced along w), both in strides of the grid.  It issues the N loads of its column (stride V H W) before it uses any and
// keeps the column in x[0 .. M), M the next multiple of 4 from N (one kernel per M: 16 of them), the rest +inf.
//
// Mean and spread read x in member order, before the sort: s += x_m; mean64 = s / N; v += (x_m - mean64)^2, difference, product
// and sum rounded separately; sqrt(v / (N - 1)).  Equal members give N x exactly (N <= 64), hence mean x and spread 0.0.
//
// Quantiles: the network above (v_min / v_max pairs; IEEE comparison, so -0 ties with +0 and either may come first; NaN is not
// detected) sorts x ascending, the padding stays on top and is never picked: the table's index is clamped into [0, N - 1].
// The network is what the call costs beyond its bytes (measured at 12 members: 0.26 ms without quantiles, 0.37 ms with the 80
// exchanges of a bitonic sort of 16): hence one cut to the multiple of 4, not one per power of two.  Quantile j is a + g (b - a)
// with a = x_(lo), b = x_(min(lo + 1, N - 1)), g = q_frac[j]: difference, product and sum each rounded to fp64, then one cast;
// g = 0 gives a exactly.
//
// Every (statistic, pixel) of out is written by exactly one thread: no atomics, no clearing.
template <int P, int M>
__global__ __launch_bounds__(256) static void ensemble_summary_kernel(const float* __restrict__ pred, const int* __restrict__ q_lo,
                                                                      const double* __restrict__ q_frac, float* __restrict__ out,
                                                                      int N, int V, int H, int W, int Q, int64_t planes) {
    const int64_t hw = (int64_t)H * W, sstride = (int64_t)V * hw;  // members, and statistics, lie V H W floats apart
    const double dn = (double)N, dn1 = (double)(N - 1);
    for (int64_t plane = blockIdx.x; plane < planes; plane += gridDim.x) {
        const int64_t i = plane / V, v = plane - i * V;
        const float* xp = pred + (i * N * V + v) * hw;
        float* op = out + (i * (2 + Q) * V + v) * hw;
        for (int64_t at = (int64_t)blockIdx.y * 256 + threadIdx.x; at < hw; at += (int64_t)gridDim.y * 256) {
            float x[M];   // (M - 4 < N <= M, and N is uniform: no lane diverges)
#pragma unroll
            for (int m = 0; m < M; ++m) x[m] = (m <= M - 4 || m < N) ? xp[at + m * sstride] : INFINITY;
            double s = 0.0;
#pragma unroll
            for (int m = 0; m < M; ++m)
                if (m <= M - 4 || m < N) s = dadd_rn(s, (double)x[m]);
            const double mean = __ddiv_rn(s, dn);
            double var = 0.0;
#pragma unroll
            for (int m = 0; m < M; ++m) {
                if (m <= M - 4 || m < N) {
                    const double d = dsub_rn((double)x[m], mean);
                    var = dadd_rn(var, dmul_rn(d, d));
                }
            }
            op[at] = (float)mean;
            op[at + sstride] = (float)__dsqrt_rn(__ddiv_rn(var, dn1));
            if (Q > 0) {
                sort_ascending<P, M>(x, std::make_integer_sequence<int, kSortNet<P, M>.n>{});
                for (int j = 0; j < Q; ++j) {
                    int lo = q_lo[j];
                    lo = lo < 0 ? 0 : lo > N - 1 ? N - 1 : lo;
                    const int up = lo + 1 > N - 1 ? N - 1 : lo + 1;
                    const double a = (double)pick<M>(x, lo), b = (double)pick<M>(x, up);
                    op[at + (2 + j) * sstride] = (float)dadd_rn(a, dmul_rn(q_frac[j], dsub_rn(b, a)));
                }
            }
        }
    }
}

extern "C" int swiftk_ensemble_summary(const float* pred, const int* q_lo, const double* q_frac, float* out, int n, int N, int V,
                                       int H, int W, int Q, void* stream) {
    if (!pred || !out || n <= 0 || N <= 0 || V <= 0 || H <= 0 || W <= 0) return SWIFTK_EINVAL;
    if (N < 2 || N > 64 || Q < 0 || Q > 16 || (int64_t)n * V > INT32_MAX) return SWIFTK_ESHAPE;
    if (Q > 0 && (!q_lo || !q_frac)) return SWIFTK_EINVAL;
    if ((((uintptr_t)pred | (uintptr_t)out | (uintptr_t)q_lo) & 3) || ((uintptr_t)q_frac & 7)) return SWIFTK_EALIGN;
    const int64_t planes = (int64_t)n * V, hw = (int64_t)H * W, chunks = (hw + 255) / 256;
    // the grid strides over planes and pixels beyond these caps (1M planes x 4096 blocks of a plane)
    const dim3 grid((unsigned)(planes < (1 << 20) ? planes : (1 << 20)), (unsigned)(chunks < 4096 ? chunks : 4096));
    hipStream_t s = static_cast<hipStream_t>(stream);
#define SWIFTK_SUMMARY_LAUNCH(P, M)                                                                                          \
    case M:                                                                                                                  \
        hipLaunchKernelGGL((ensemble_summary_kernel<P, M>), grid, dim3(256), 0, s, pred, q_lo, q_frac, out, N, V, H, W, Q, \
                           planes);                                                                                          \
        break;
    switch ((N + 3) & ~3) {  // the members padded to a multiple of 4, inside the next power of two (at least 4)
        SWIFTK_SUMMARY_LAUNCH(4, 4)
        SWIFTK_SUMMARY_LAUNCH(8, 8)
        SWIFTK_SUMMARY_LAUNCH(16, 12)
        SWIFTK_SUMMARY_LAUNCH(16, 16)
        SWIFTK_SUMMARY_LAUNCH(32, 20)
        SWIFTK_SUMMARY_LAUNCH(32, 24)
        SWIFTK_SUMMARY_LAUNCH(32, 28)
        SWIFTK_SUMMARY_LAUNCH(32, 32)
        SWIFTK_SUMMARY_LAUNCH(64, 36)
        SWIFTK_SUMMARY_LAUNCH(64, 40)
        SWIFTK_SUMMARY_LAUNCH(64, 44)
        SWIFTK_SUMMARY_LAUNCH(64, 48)
        SWIFTK_SUMMARY_LAUNCH(64, 52)
        SWIFTK_SUMMARY_LAUNCH(64, 56)
        SWIFTK_SUMMARY_LAUNCH(64, 60)
        SWIFTK_SUMMARY_LAUNCH(64, 64)
    }
#undef SWIFTK_SUMMARY_LAUNCH
    SWIFTK_CHECK_LAUNCH();
    return 0;
}
