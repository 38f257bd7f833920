// Rank (Talagrand) histograms of an ensemble against the verifying fields in fp64 (swiftk_rank_histogram, include/swiftk.h):
// the calibration evidence of `swift_amd.generate --rank-hist`.  Counting is exact integer work, floating point enters in three
// places only, so one order of arithmetic per bin serves every batch shape.
#include "common.h"

// One workgroup per (i, v) plane walks the rows in order, RT at a time, one table per row.
//
// Counting.  A thread owns columns w = tid, tid + 256, ... of every row of the group (coalesced along w), reads the truth and the
// N member values (stride V H W) of its RT pixels once -- members outside, rows inside, so RT independent loads per member and 16
// in flight per thread: the kernel lives on memory latency, 2 workgroups per CU at the workload's 552 planes (measured at 12
// members: 8 rows per group 0.24 ms, 4 rows 0.46-0.51 ms, one row's members after the other's 0.73 ms; 32 in flight: no gain) --
// and keeps b = #{x_m < y} and e = #{x_m == y} per pixel.  The pixel covers bins b .. b + e of tie size e: it adds +1 at
// D[row][e][b] and -1 at D[row][e][b + e + 1] (dropped when that is past bin N), so that the prefix sum over r of D[row][e][.] is
// T_h[e][r], the number of pixels of the row with tie size e whose range covers r.  These are integer LDS adds: exact, so their
// order does not matter.  The tie sizes that occur at all are or-ed into a 65-bit mask per row; real fields have one or two (0,
// and N on a channel forced to a constant), and only those are summed.
//
// Floating point, all fp64, thread (row, r): row[r] = sum over the present e ascending of T_h[e][r] / (e + 1) (an absent e would
// add +0.0 to a non-negative sum: skipping it leaves the bits alone); then thread r: acc[r] += w_lat[h] * row[r], rows in ascending
// h, product and sum rounded separately (no contraction: the order of arithmetic is the one documented, on any compiler).
//
// LDS (dynamic): rowv [RT][N + 1] doubles | D [RT][N + 1][N + 1] ints | mask [RT][3] words: 35 KB at N = 64 (RT = 2), 6 KB at
// N = 12 (RT = 8; RT = 4 from N = 16, 2 from N = 32).  acc[r] lives in a register of thread r.  The bits of a plane's bins depend on
// (N, H, W), the weights and the plane's values only.
template <int RT>
__global__ __launch_bounds__(256) static void rank_histogram_kernel(const float* __restrict__ pred, const float* __restrict__ y,
                                                                    const double* __restrict__ w_lat, double* __restrict__ out,
                                                                    int N, int V, int H, int W) {
    extern __shared__ double rh_lds[];
    constexpr int UNR = 16 / RT;  // members per trip of the load loop: 16 loads in flight per thread
    const int B = N + 1, tab = B * B;
    double* rowv = rh_lds;
    int* D = reinterpret_cast<int*>(rowv + RT * B);
    unsigned* mask = reinterpret_cast<unsigned*>(D + RT * tab);
    constexpr int T = 256;  // the launch's block size
    const int tid = threadIdx.x;
    const int64_t plane = blockIdx.x, i = blockIdx.x / (unsigned)V, v = plane - i * V;  // (n V fits 31 bits)
    const int64_t hw = (int64_t)H * W, mstride = (int64_t)V * hw;
    const float* xp = pred + (i * N * V + v) * hw;  // member 0 of this plane; member m lies m * mstride further on
    const float* yp = y + plane * hw;

    for (int j = tid; j < RT * tab; j += T) D[j] = 0;
    if (tid < RT * 3) mask[tid] = 0u;
    double acc = 0.0;

    for (int h0 = 0; h0 < H; h0 += RT) {
        const int rows = H - h0 < RT ? H - h0 : RT;
        __syncthreads();  // tables and masks are clear
        for (int64_t w = tid; w < W; w += T) {
            // a row past the end of the plane is read as the group's last row and dropped below: the loads stay unconditional
            int64_t q[RT];  // (indices off the one global pointer, not pointers: an array of those is loaded from as generic)
            float yv[RT];
            int b[RT], e[RT];
            int64_t at = (int64_t)h0 * W + w;
#pragma unroll
            for (int t = 0; t < RT; ++t) {
                if (t > 0 && t < rows) at += W;
                q[t] = at;
                yv[t] = yp[at];
                b[t] = e[t] = 0;
            }
            // members outside, rows inside: RT independent loads per member, 16 in flight per thread with the unrolling
#pragma unroll UNR
            for (int m = 0; m < N; ++m) {
#pragma unroll
                for (int t = 0; t < RT; ++t) {
                    const float x = xp[q[t]];
                    q[t] += mstride;
                    b[t] += x < yv[t];
                    e[t] += x == yv[t];
                }
            }
#pragma unroll
            for (int t = 0; t < RT; ++t) {
                if (t < rows) {
                    int* d = D + t * tab + e[t] * B;
                    atomicAdd(d + b[t], 1);
                    if (b[t] + e[t] < N) atomicAdd(d + b[t] + e[t] + 1, -1);
                    atomicOr(mask + t * 3 + (e[t] >> 5), 1u << (e[t] & 31));
                }
            }
        }
        __syncthreads();
        if (tid < rows * B) {
            const int t = tid / B, r = tid - t * B;
            double s = 0.0;
            for (int word = 0; word < 3; ++word) {
                unsigned m = mask[t * 3 + word];
                while (m) {
                    const int e = word * 32 + __ffs(m) - 1;
                    m &= m - 1;
                    const int* d = D + t * tab + e * B;
                    int c = 0;
                    for (int j = 0; j <= r; ++j) c += d[j];
                    s = __dadd_rn(s, __ddiv_rn((double)c, (double)(e + 1)));
                }
            }
            rowv[tid] = s;
        }
        __syncthreads();  // the row sums are in place and the tables have been read
        if (tid < B) {
            for (int t = 0; t < rows; ++t) acc = __dadd_rn(acc, __dmul_rn(w_lat[h0 + t], rowv[t * B + tid]));
        }
        for (int j = tid; j < RT * tab; j += T) D[j] = 0;
        if (tid < RT * 3) mask[tid] = 0u;
    }
    if (tid < B) out[plane * B + tid] = acc;
}

extern "C" int swiftk_rank_histogram(const float* pred, const float* y, const double* w_lat, double* out, int n, int N, int V,
                                     int H, int W, void* stream) {
    if (!pred || !y || !w_lat || !out || n <= 0 || N <= 0 || V <= 0 || H <= 0 || W <= 0) return SWIFTK_EINVAL;
    if (N > 64 || (int64_t)n * V > INT32_MAX) return SWIFTK_ESHAPE;
    if ((((uintptr_t)pred | (uintptr_t)y) & 3) || (((uintptr_t)w_lat | (uintptr_t)out) & 7)) return SWIFTK_EALIGN;
    const int rt = N <= 15 ? 8 : N <= 31 ? 4 : 2;  // rows per group: rt * (N + 1) threads fill the row sums (<= 130), rt tables <= 35 KB
    const int B = N + 1;
    const size_t lds = (size_t)rt * B * sizeof(double) + (size_t)rt * B * B * sizeof(int) + (size_t)rt * 3 * sizeof(unsigned);
    const dim3 grid((unsigned)((int64_t)n * V));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (rt == 8)
        hipLaunchKernelGGL(rank_histogram_kernel<8>, grid, dim3(256), lds, s, pred, y, w_lat, out, N, V, H, W);
    else if (rt == 4)
        hipLaunchKernelGGL(rank_histogram_kernel<4>, grid, dim3(256), lds, s, pred, y, w_lat, out, N, V, H, W);
    else
        hipLaunchKernelGGL(rank_histogram_kernel<2>, grid, dim3(256), lds, s, pred, y, w_lat, out, N, V, H, W);
    SWIFTK_CHECK_LAUNCH();
    return 0;
}
