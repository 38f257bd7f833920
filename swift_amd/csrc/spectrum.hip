// Zonal power spectra of field planes in fp64 (swiftk_zonal_power, include/swiftk.h): the sharpness evidence of
// `swift_amd.generate --spectra`.  A direct transform, not an FFT: W need not be a power of two, the planes are small
// (128 x 256) and there are thousands of them, and a direct sum has one fixed order of additions per bin.
#include "common.h"

// One workgroup per (n, v) plane walks the rows in order, RT at a time.  A row group is widened to fp64 (the mean over
// the G member planes first, members added in member order) into LDS as xs[w][r]; thread k then carries bin k of every row of
// the group through the W terms -- one table entry (k w) mod W feeds 2 RT multiply-adds, the row values are broadcast reads.
//
// Bins 0 and W/2 are real sums (sum_w x and sum_w (-1)^w x) and share thread 0: its "table" is the two extra entries
// tab[W] = (1, 1), tab[W + 1] = (1, -1), walked with step 1 and wrap 2, so that its real part is bin 0 and its imaginary part is
// bin W/2 and the threads 0 .. W/2 - 1 cover all W/2 + 1 bins with the same loop body.
//
// LDS (dynamic, doubles): tab [W + 2][2] | xs [W][RT] (RT W <= 2048) | acc [W/2 + 1]: 56 KB at W = 2048, 22 KB at W = 256.
// acc[k] is read and written by the one thread that owns bin k; rows are added in row order, so the bits of a plane's spectrum
// depend on (G, H, W) and the plane's values only.
template <int RT>
__global__ __launch_bounds__(256) static void zonal_power_kernel(const float* __restrict__ x, const double* __restrict__ w_lat,
                                                                 const double* __restrict__ twiddle, double* __restrict__ out,
                                                                 int G, int V, int H, int W, double inv_g) {
    extern __shared__ double2 zp_lds[];
    double2* tab = zp_lds;
    double* xs = reinterpret_cast<double*>(tab + W + 2);
    double* acc = xs + RT * W;
    const int tid = threadIdx.x, T = blockDim.x, half = W >> 1;
    const int64_t plane = blockIdx.x, n = plane / V, v = plane - n * V;
    const int64_t hw = (int64_t)H * W, gstride = (int64_t)V * hw;
    const float* xp = x + (n * G * V + v) * hw;  // member 0 of this plane; member g lies g * gstride further on

    for (int j = tid; j < W; j += T) tab[j] = make_double2(twiddle[2 * j], twiddle[2 * j + 1]);
    if (tid == 0) {
        tab[W] = make_double2(1.0, 1.0);
        tab[W + 1] = make_double2(1.0, -1.0);
    }
    for (int k = tid; k <= half; k += T) acc[k] = 0.0;

    for (int h0 = 0; h0 < H; h0 += RT) {
        __syncthreads();  // the previous group has been read (first pass: table and acc are in place)
        for (int e = tid; e < RT * W; e += T) {
            const int r = e / W, w = e - r * W, h = h0 + r;
            double s = 0.0;
            if (h < H) {
                const float* p = xp + (int64_t)h * W + w;
                s = (double)p[0];
                for (int g = 1; g < G; ++g) s += (double)p[g * gstride];
                if (G > 1) s *= inv_g;
            }
            xs[w * RT + r] = s;
        }
        __syncthreads();
        for (int k = tid; k < half; k += T) {
            const int base = k ? 0 : W, wrap = k ? W : 2, step = k ? k : 1;
            double re[RT], im[RT];  // (im carries + sum x sin: the sign does not reach the power)
#pragma unroll
            for (int r = 0; r < RT; ++r) re[r] = im[r] = 0.0;
            int idx = 0;
            for (int w = 0; w < W; ++w) {
                const double2 t = tab[base + idx];
#pragma unroll
                for (int r = 0; r < RT; ++r) {
                    const double xv = xs[w * RT + r];
                    re[r] = fma(xv, t.x, re[r]);
                    im[r] = fma(xv, t.y, im[r]);
                }
                idx += step;
                if (idx >= wrap) idx -= wrap;
            }
            double a = acc[k], a_nyq = k ? 0.0 : acc[half];
#pragma unroll
            for (int r = 0; r < RT; ++r) {
                if (h0 + r < H) {
                    const double wl = w_lat[h0 + r];
                    if (k) {
                        a += wl * (re[r] * re[r] + im[r] * im[r]);
                    } else {
                        a += wl * (re[r] * re[r]);
                        a_nyq += wl * (im[r] * im[r]);
                    }
                }
            }
            acc[k] = a;
            if (!k) acc[half] = a_nyq;
        }
    }
    const double norm = (double)W * (double)W * (double)H;
    double* o = out + plane * (half + 1);
    for (int k = tid; k < half; k += T) o[k] = (k ? 2.0 : 1.0) * acc[k] / norm;
    if (tid == 0) o[half] = acc[half] / norm;
}

extern "C" int swiftk_zonal_power(const float* x, const double* w_lat, const double* twiddle, double* out, int n, int G, int V,
                                  int H, int W, void* stream) {
    if (!x || !w_lat || !twiddle || !out || n <= 0 || G <= 0 || V <= 0 || H <= 0 || W <= 0) return SWIFTK_EINVAL;
    if ((W & 1) || W < 4 || W > 2048 || (int64_t)n * V > INT32_MAX) return SWIFTK_ESHAPE;
    if (((uintptr_t)x & 3) || (((uintptr_t)w_lat | (uintptr_t)twiddle | (uintptr_t)out) & 7)) return SWIFTK_EALIGN;
    const int half = W / 2, threads = half >= 256 ? 256 : (half + 63) / 64 * 64;
    const int rt = W <= 256 ? 8 : W <= 512 ? 4 : W <= 1024 ? 2 : 1;  // rows per group: rt * W <= 2048 doubles of LDS
    const size_t lds = ((size_t)(W + 2) * 2 + (size_t)rt * W + half + 1) * sizeof(double);
    const dim3 grid((unsigned)((int64_t)n * V));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const double inv_g = 1.0 / (double)G;
    switch (rt) {
        case 8: hipLaunchKernelGGL(zonal_power_kernel<8>, grid, dim3(threads), lds, s, x, w_lat, twiddle, out, G, V, H, W, inv_g); break;
        case 4: hipLaunchKernelGGL(zonal_power_kernel<4>, grid, dim3(threads), lds, s, x, w_lat, twiddle, out, G, V, H, W, inv_g); break;
        case 2: hipLaunchKernelGGL(zonal_power_kernel<2>, grid, dim3(threads), lds, s, x, w_lat, twiddle, out, G, V, H, W, inv_g); break;
        default: hipLaunchKernelGGL(zonal_power_kernel<1>, grid, dim3(threads), lds, s, x, w_lat, twiddle, out, G, V, H, W, inv_g);
    }
    SWIFTK_CHECK_LAUNCH();
    return 0;
}
