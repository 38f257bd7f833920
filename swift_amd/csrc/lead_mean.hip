// Means over lead-time windows (swiftk_lead_window_mean, include/swiftk.h): x [n, M] -> out [nw, M], window w the mean of the lead
// rows first[w] .. first[w] + count[w] - 1 of every column -- the week-1 / week-2 / weeks 3-4 fields that `swift_amd.generate
// --lead-windows` scores.  fp64 running sums in lead order, one division, one cast: one set of bits per column whatever the shape.
#include "common.h"

#include <limits.h>
#include <math.h>

// A rounded fp64 add that stays an add (ensemble_summary.hip: the plain operator, and hipcc's __dadd_rn, may be contracted).
static __device__ __forceinline__ double dadd_rn(double x, double y) { return __ocml_add_rte_f64(x, y); }

#define SWIFTK_LEAD_MAX_WINDOWS 8
#define SWIFTK_LEAD_COLS 4

// The call's windows by value, in the kernel's arguments: window w covers the rows [first, end); a slot past the call's windows
// holds first = end = -1 and matches no row.  The rows that lie in any window, ascending, are numbered 0 .. total - 1: they form
// at most nw runs of consecutive rows, run q beginning at number start[q] (INT_MAX for a slot without a run; start[0] = 0), and a
// row of run q is its number plus delta[q].
struct LeadWindows {
    int first[SWIFTK_LEAD_MAX_WINDOWS];
    int end[SWIFTK_LEAD_MAX_WINDOWS];
    int start[SWIFTK_LEAD_MAX_WINDOWS];
    int delta[SWIFTK_LEAD_MAX_WINDOWS];
    int total;
};

// B consecutive wanted rows from number i0 on: their B x 16 bytes per thread are requested before any is used -- the kernel
// streams, and like ensemble_maps.hip and rank_hist.hip it lives on the loads in flight -- then row by row, window by window:
// the window's first row sets the running sum, a later one adds to it.  Rows and windows are uniform scalars, every test on
// them unrolled; s[w][k] is never indexed at run time.
template <int NW, bool VEC, int B>
static __device__ __forceinline__ void lead_rows(const float* __restrict__ x, const LeadWindows& win, int i0, int64_t M,
                                                 const int64_t (&col)[SWIFTK_LEAD_COLS], double (&s)[NW][SWIFTK_LEAD_COLS]) {
    constexpr int COLS = SWIFTK_LEAD_COLS;
    int r[B];
    float v[B][COLS];
#pragma unroll
    for (int j = 0; j < B; ++j) {
        int d = win.delta[0];
#pragma unroll
        for (int q = 1; q < NW; ++q) d = i0 + j >= win.start[q] ? win.delta[q] : d;
        r[j] = i0 + j + d;
        const float* row = x + (int64_t)r[j] * M;
        if (VEC) {
            const float4 q4 = *reinterpret_cast<const float4*>(row + col[0]);
            v[j][0] = q4.x, v[j][1] = q4.y, v[j][2] = q4.z, v[j][3] = q4.w;
        } else {
#pragma unroll
            for (int k = 0; k < COLS; ++k) v[j][k] = row[col[k]];
        }
    }
#pragma unroll
    for (int j = 0; j < B; ++j) {
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            if (r[j] == win.first[w]) {
#pragma unroll
                for (int k = 0; k < COLS; ++k) s[w][k] = (double)v[j][k];
            } else if (r[j] > win.first[w] && r[j] < win.end[w]) {
#pragma unroll
                for (int k = 0; k < COLS; ++k) s[w][k] = dadd_rn(s[w][k], (double)v[j][k]);
            }
        }
    }
}

// A thread owns 4 columns: VEC, 4 neighbours read and written as one 16-byte access (x and out on 16-byte boundaries, M a multiple
// of 4, so every row is); otherwise 4 columns 256 apart, a dword each (every load and store coalesced either way).  A block takes
// 1024 columns and strides over the columns in steps of the grid.  The thread walks the wanted lead rows once, in order, 8 at a
// time (32 KiB of loads in flight per block), the last 7 or fewer as 4, 2 and 1: a row that lies in no window is not read, one in
// several windows is read once.  The running sums are NW x 4 fp64 registers.  A column past M is read as the last one and not
// stored: the loads stay unconditional and in bounds.
//
// Per column and window: s = (double)x[first]; s = s (+) (double)x[r] for r ascending, one rounded add each; out = (float)(s /
// (double)count).  The sum starts from the first element, so a window of one row returns its input bits.  Every element of out
// belongs to exactly one thread: no atomics, no scratch, no clearing.
template <int NW, bool VEC>
__global__ __launch_bounds__(256) static void lead_window_mean_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                                      const LeadWindows win, int nw, int64_t M) {
    constexpr int COLS = SWIFTK_LEAD_COLS;
    const int64_t chunk = 256 * COLS;
    for (int64_t c0 = (int64_t)blockIdx.x * chunk; c0 < M; c0 += (int64_t)gridDim.x * chunk) {
        int64_t col[COLS];   // VEC: col[0] the first of the thread's 4 neighbours
        bool live[COLS];
        if (VEC) {
            const int64_t c = c0 + (int64_t)threadIdx.x * COLS;
            live[0] = c < M;
            col[0] = live[0] ? c : M - COLS;
        } else {
#pragma unroll
            for (int k = 0; k < COLS; ++k) {
                const int64_t c = c0 + k * 256 + threadIdx.x;
                live[k] = c < M;
                col[k] = live[k] ? c : M - 1;
            }
        }
        double s[NW][COLS];
#pragma unroll
        for (int w = 0; w < NW; ++w)
#pragma unroll
            for (int k = 0; k < COLS; ++k) s[w][k] = 0.0;
        int i = 0;
        for (; i + 8 <= win.total; i += 8) lead_rows<NW, VEC, 8>(x, win, i, M, col, s);
        if (i + 4 <= win.total) {
            lead_rows<NW, VEC, 4>(x, win, i, M, col, s);
            i += 4;
        }
        if (i + 2 <= win.total) {
            lead_rows<NW, VEC, 2>(x, win, i, M, col, s);
            i += 2;
        }
        if (i < win.total) lead_rows<NW, VEC, 1>(x, win, i, M, col, s);
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            if (w < nw) {
                const double cnt = (double)(win.end[w] - win.first[w]);
                float* row = out + (int64_t)w * M;
                if (VEC) {
                    if (live[0])
                        *reinterpret_cast<float4*>(row + col[0]) =
                            make_float4((float)__ddiv_rn(s[w][0], cnt), (float)__ddiv_rn(s[w][1], cnt),
                                        (float)__ddiv_rn(s[w][2], cnt), (float)__ddiv_rn(s[w][3], cnt));
                } else {
#pragma unroll
                    for (int k = 0; k < COLS; ++k)
                        if (live[k]) row[col[k]] = (float)__ddiv_rn(s[w][k], cnt);
                }
            }
        }
    }
}

extern "C" int swiftk_lead_window_mean(const float* x, float* out, const int* first, const int* count, int n, int nw, int64_t M,
                                       void* stream) {
    if (!x || !out || !first || !count || n <= 0 || nw <= 0 || M <= 0) return SWIFTK_EINVAL;
    if (nw > SWIFTK_LEAD_MAX_WINDOWS) return SWIFTK_ESHAPE;
    LeadWindows win;
    for (int w = 0; w < SWIFTK_LEAD_MAX_WINDOWS; ++w) {
        win.first[w] = win.end[w] = -1;
        win.start[w] = INT_MAX, win.delta[w] = 0;
        if (w < nw) {
            if (first[w] < 0 || count[w] < 1 || (int64_t)first[w] + count[w] > n) return SWIFTK_ESHAPE;
            win.first[w] = first[w], win.end[w] = first[w] + count[w];
        }
    }
    if (((uintptr_t)x | (uintptr_t)out) & 3) return SWIFTK_EALIGN;
    // the runs of rows that lie in any window, ascending: each starts at the smallest window start not yet covered and grows
    // while some window starts inside it or right behind it
    int runs = 0, covered = 0;  // rows below `covered` are dealt with
    win.total = 0;
    for (;;) {
        int lo = INT_MAX;
        for (int w = 0; w < nw; ++w)
            if (win.end[w] > covered && win.first[w] < lo) lo = win.first[w];  // (no window straddles `covered`)
        if (lo == INT_MAX) break;
        int hi = lo;
        for (bool grown = true; grown;) {
            grown = false;
            for (int w = 0; w < nw; ++w)
                if (win.first[w] <= hi && win.end[w] > hi) hi = win.end[w], grown = true;
        }
        win.start[runs] = win.total, win.delta[runs] = lo - win.total;
        win.total += hi - lo;
        covered = hi;
        ++runs;
    }
    const bool vec = !(((uintptr_t)x | (uintptr_t)out) & 15) && M % 4 == 0;
    const int64_t chunks = (M + 1023) / 1024;
    const dim3 grid((unsigned)(chunks < 2048 ? chunks : 2048));  // the grid strides over the columns beyond 2048 blocks of 1024
    hipStream_t s = static_cast<hipStream_t>(stream);
#define SWIFTK_LEAD_LAUNCH(NW_)                                                                                   \
    if (vec)                                                                                                      \
        hipLaunchKernelGGL((lead_window_mean_kernel<NW_, true>), grid, dim3(256), 0, s, x, out, win, nw, M);   \
    else                                                                                                          \
        hipLaunchKernelGGL((lead_window_mean_kernel<NW_, false>), grid, dim3(256), 0, s, x, out, win, nw, M);
    if (nw == 1) {  // one kernel per 1, 2, 4 and 8 window slots: an empty slot costs its scalar tests only
        SWIFTK_LEAD_LAUNCH(1)
    } else if (nw == 2) {
        SWIFTK_LEAD_LAUNCH(2)
    } else if (nw <= 4) {
        SWIFTK_LEAD_LAUNCH(4)
    } else {
        SWIFTK_LEAD_LAUNCH(8)
    }
#undef SWIFTK_LEAD_LAUNCH
    SWIFTK_CHECK_LAUNCH();
    return 0;
}
