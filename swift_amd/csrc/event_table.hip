// Contingency tables of threshold events, ensemble against verifying fields, in fp64 (swiftk_event_table, include/swiftk.h): the
// Brier score and reliability evidence of `swift_amd.generate --events`.  Counting is exact integer work, floating point enters
// once, so one order of arithmetic per cell serves every batch shape.
#include "common.h"

// One workgroup per (i, e) plane walks the rows in order, RT at a time, one table per row (the structure of rank_hist.hip).
//
// Counting.  A thread owns columns w = tid, tid + 256, ... of every row of the group (coalesced along w), reads the threshold, the
// truth and the N member values (stride V H W) of its RT pixels once -- members outside, rows inside, so RT independent loads per
// member and 16 in flight per thread: the kernel lives on memory latency, as the rank histogram does -- and keeps k = #{m :
// event(x_m)} per pixel.  A pixel whose threshold is not NaN adds 1 at C[row][k][o], o = event(y): one integer LDS add (the rank
// histogram needs three), exact, so the order does not matter.  Both comparisons are strict IEEE compares of the fp32 values as
// loaded (no sign flip, no arithmetic on them): x == t is no event, -0 == +0.
//
// Floating point, all fp64: thread (k, o) adds w_lat[h] * (double)C[row][k][o] to its register, rows in ascending h, product and
// sum rounded separately (no contraction: the order of arithmetic is the one documented, on any compiler), and clears the cell it
// has just read.
//
// LDS (dynamic): C [RT][N + 1][2] ints: 4160 B at N = 64, so RT = 8 rows at every N.  The bits of a plane's table depend on (N, H,
// W), the weights, the threshold field and the plane's values only.
constexpr int ET_RT = 8;     // rows per group
constexpr int ET_T = 256;    // the launch's block size: 2 (N + 1) <= 130 of its threads own a cell

__global__ __launch_bounds__(ET_T) static void event_table_kernel(const float* __restrict__ pred, const float* __restrict__ y,
                                                                  const float* __restrict__ thr, const int* __restrict__ ev_var,
                                                                  const int* __restrict__ ev_dir, const double* __restrict__ w_lat,
                                                                  double* __restrict__ out, int N, int V, int H, int W, int E) {
    extern __shared__ int et_lds[];
    constexpr int RT = ET_RT, T = ET_T;
    constexpr int UNR = 16 / RT;  // members per trip of the load loop: 16 loads in flight per thread
    const int cells = 2 * (N + 1);
    int* C = et_lds;
    const int tid = threadIdx.x;
    const int64_t plane = blockIdx.x, i = blockIdx.x / (unsigned)E, e = plane - i * E;  // (n E fits 31 bits)
    int v = ev_var[e];
    v = v < 0 ? 0 : v > V - 1 ? V - 1 : v;  // read on the device, so it could not be refused before the launch: clamped
    const bool lt = ev_dir[e] != 0;
    const int64_t hw = (int64_t)H * W, mstride = (int64_t)V * hw;
    const float* xp = pred + (i * N * V + v) * hw;  // member 0 of the event's channel; member m lies m * mstride further on
    const float* yp = y + (i * V + v) * hw;
    const float* tp = thr + e * hw;

    for (int j = tid; j < RT * cells; j += T) C[j] = 0;
    double acc = 0.0;

    for (int h0 = 0; h0 < H; h0 += RT) {
        const int rows = H - h0 < RT ? H - h0 : RT;
        __syncthreads();  // the tables are clear
        for (int64_t w = tid; w < W; w += T) {
            // a row past the end of the plane is read as the group's last row and dropped below: the loads stay unconditional
            int64_t q[RT];  // (indices off the one global pointer, not pointers: an array of those is loaded from as generic)
            float tv[RT], yv[RT];
            int k[RT];
            int64_t at = (int64_t)h0 * W + w;
#pragma unroll
            for (int t = 0; t < RT; ++t) {
                if (t > 0 && t < rows) at += W;
                q[t] = at;
                tv[t] = tp[at];
                yv[t] = yp[at];
                k[t] = 0;
            }
            // members outside, rows inside: RT independent loads per member, 16 in flight per thread with the unrolling
#pragma unroll UNR
            for (int m = 0; m < N; ++m) {
#pragma unroll
                for (int t = 0; t < RT; ++t) {
                    const float x = xp[q[t]];
                    q[t] += mstride;
                    k[t] += lt ? x < tv[t] : x > tv[t];
                }
            }
#pragma unroll
            for (int t = 0; t < RT; ++t) {
                if (t < rows && tv[t] == tv[t]) {  // a NaN threshold masks the pixel out of every cell
                    const int o = lt ? yv[t] < tv[t] : yv[t] > tv[t];
                    atomicAdd(C + t * cells + k[t] * 2 + o, 1);
                }
            }
        }
        __syncthreads();
        if (tid < cells) {
            // (__dmul_rn and __dadd_rn are inline * and + to this compiler and fuse once inlined: the operators are written out
            // under the pragma, which takes the permission to contract off them)
#pragma clang fp contract(off)
            for (int t = 0; t < rows; ++t) {
                const double term = w_lat[h0 + t] * (double)C[t * cells + tid];
                acc = acc + term;
                C[t * cells + tid] = 0;  // this thread's own cell: clear for the next group after the barrier at the loop's top
            }
        }
    }
    if (tid < cells) out[plane * cells + tid] = acc;
}

extern "C" int swiftk_event_table(const float* pred, const float* y, const float* thr, const int* ev_var, const int* ev_dir,
                                  const double* w_lat, double* out, int n, int N, int V, int H, int W, int E, void* stream) {
    if (!pred || !y || !thr || !ev_var || !ev_dir || !w_lat || !out || n <= 0 || N <= 0 || V <= 0 || H <= 0 || W <= 0 || E <= 0)
        return SWIFTK_EINVAL;
    if (N > 64 || (int64_t)n * E > INT32_MAX) return SWIFTK_ESHAPE;
    if ((((uintptr_t)pred | (uintptr_t)y | (uintptr_t)thr | (uintptr_t)ev_var | (uintptr_t)ev_dir) & 3) ||
        (((uintptr_t)w_lat | (uintptr_t)out) & 7))
        return SWIFTK_EALIGN;
    const size_t lds = (size_t)ET_RT * 2 * (N + 1) * sizeof(int);
    const dim3 grid((unsigned)((int64_t)n * E));
    hipLaunchKernelGGL(event_table_kernel, grid, dim3(ET_T), lds, static_cast<hipStream_t>(stream), pred, y, thr, ev_var, ev_dir,
                       w_lat, out, N, V, H, W, E);
    SWIFTK_CHECK_LAUNCH();
    return 0;
}
