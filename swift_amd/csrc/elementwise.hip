// HBM-bound pieces of the SwinV2 forecast path for gfx950: modulated LayerNorm + residual,
// patchify / un-patchify with the concat and the sampler update folded in, the tiny
// time-embedding MLP, the rollout state update and operand casts.
#include "common.h"
#include <type_traits>

int g_modnorm_nt = 3;  // tuning key 6: bit 0 = stream the fp32 residual with non-temporal loads / stores, bit 1 = chunked kernel,
                       // bit 2 = row-per-wave pair kernel instead of the packed one (A/B)

namespace {

// --------------------------------------------------------------------------------- modnorm + residual
// One wave per token row, 8 channels per lane per slot (16 B of bf16 y / 32 B of fp32).  All y and x loads of a
// row are issued before the first reduction so ~5 KiB per wave is in flight; the row lives in registers
// between the two reduction passes (exact two-pass variance).  Bytes per element: read y (2|4) + x (4),
// write x (4) + operand copy (2|4).
// streaming (non-temporal) forms for the fp32 residual stream: read once, written once, not needed again for a whole
// GEMM + attention -- keeping it out of the way leaves L2 / Infinity Cache to the operand copy the next GEMM reads
__device__ __forceinline__ void load8_nt(const float* p, float (&v)[8]) {
    typedef __attribute__((ext_vector_type(4))) float v4;
    const v4 a = __builtin_nontemporal_load(reinterpret_cast<const v4*>(p));
    const v4 b = __builtin_nontemporal_load(reinterpret_cast<const v4*>(p + 4));
    v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
}
__device__ __forceinline__ void store8_nt(float* p, const float (&v)[8]) {
    typedef __attribute__((ext_vector_type(4))) float v4;
    __builtin_nontemporal_store(v4{v[0], v[1], v[2], v[3]}, reinterpret_cast<v4*>(p));
    __builtin_nontemporal_store(v4{v[4], v[5], v[6], v[7]}, reinterpret_cast<v4*>(p + 4));
}

template <typename T, int SLOTS>
__global__ __launch_bounds__(256) void modnorm_kernel(const T* __restrict__ y, int64_t ldy, float* __restrict__ x,
                                                      T* __restrict__ xc, int64_t ldc, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, const float* __restrict__ mod,
                                                      int64_t ldmod, int64_t M, int d, int64_t rps, float eps, int nt_x) {
    const bool NT_X = nt_x != 0;
    const int lane = threadIdx.x & 63;
    const int nc = d >> 3;  // 8-channel slots per row
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t row = wave; row < M; row += nwaves) {
        float v[SLOTS][8], xr[SLOTS][8];
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            const int c = lane + 64 * i;
            if (c < nc) {
                load8<T>(y + row * ldy + 8 * c, v[i]);
                if (NT_X) load8_nt(x + row * d + 8 * c, xr[i]); else load8<float>(x + row * d + 8 * c, xr[i]);
            }
        }
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < SLOTS; ++i)
            if (lane + 64 * i < nc)
                sum += ((v[i][0] + v[i][1]) + (v[i][2] + v[i][3])) + ((v[i][4] + v[i][5]) + (v[i][6] + v[i][7]));
        const float mean = wave_sum(sum) / (float)d;
        float sq = 0.f;
#pragma unroll
        for (int i = 0; i < SLOTS; ++i)
            if (lane + 64 * i < nc) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    v[i][e] -= mean;
                    sq += v[i][e] * v[i][e];
                }
            }
        const float rstd = rsqrtf(wave_sum(sq) / (float)d + eps);
        const float* mrow = mod + (row / rps) * ldmod;
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            const int c = lane + 64 * i;
            if (c < nc) {
                float g[8], bt[8], sc[8], sh[8];
                load8<float>(gamma + 8 * c, g);
                load8<float>(beta + 8 * c, bt);
                load8<float>(mrow + 8 * c, sc);
                load8<float>(mrow + d + 8 * c, sh);
#pragma unroll
                for (int e = 0; e < 8; ++e) xr[i][e] += (v[i][e] * rstd * g[e] + bt[e]) * (1.0f + sc[e]) + sh[e];
                if (NT_X) store8_nt(x + row * d + 8 * c, xr[i]); else store8<float>(x + row * d + 8 * c, xr[i]);
                if (xc) store8<T>(xc + row * ldc + 8 * c, xr[i]);
            }
        }
    }
}


// Chunked form (tuning key 6 bit 1, the default): a workgroup owns MN_ROWS consecutive token rows, wave w of it the rows
// w, w + 4, ...  The per-sample modulation and the LayerNorm affine are folded ONCE per wave and sample into
//   P = gamma (1 + scale),  Q = beta (1 + scale) + shift        (x += LN(y) P + Q)
// and stay in registers across the wave's rows -- the row-per-wave form re-reads 17 KB of parameters through L1 / L2 for
// every 12.7 KB row it moves -- and the loads of the wave's next row are issued before the current row is reduced, so
// every wave keeps two rows (12.7 KB) in flight.
#ifndef SWIFTK_MN_ROWS
#define SWIFTK_MN_ROWS 16
#endif
constexpr int MN_ROWS = SWIFTK_MN_ROWS;
#ifndef SWIFTK_MNPK_OCC
#define SWIFTK_MNPK_OCC 2
#endif
#ifndef SWIFTK_MNP_OCC
#define SWIFTK_MNP_OCC 3  // pair kernel: 168 VGPRs = three waves per SIMD
#endif
#ifndef SWIFTK_MN_OCC
#define SWIFTK_MN_OCC 2
#endif

// raw 8-channel slot of y as loaded (bf16: 16 B, fp32: 32 B); unpacked only when the row is reduced, so a row waiting in
// flight costs half the registers
template <typename T> struct raw8;
template <> struct raw8<bf16_t> { uint4 q; };
template <> struct raw8<float> { float4 a, b; };
__device__ __forceinline__ void load_raw(const bf16_t* p, raw8<bf16_t>& r) { r.q = *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ void load_raw(const float* p, raw8<float>& r) {
    r.a = *reinterpret_cast<const float4*>(p);
    r.b = *reinterpret_cast<const float4*>(p + 4);
}
__device__ __forceinline__ void unpack_raw(const raw8<bf16_t>& r, float (&v)[8]) {
    const uint32_t u[4] = {r.q.x, r.q.y, r.q.z, r.q.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[2 * e] = __uint_as_float(u[e] << 16);
        v[2 * e + 1] = __uint_as_float(u[e] & 0xffff0000u);
    }
}
__device__ __forceinline__ void unpack_raw(const raw8<float>& r, float (&v)[8]) {
    v[0] = r.a.x; v[1] = r.a.y; v[2] = r.a.z; v[3] = r.a.w; v[4] = r.b.x; v[5] = r.b.y; v[6] = r.b.z; v[7] = r.b.w;
}

template <typename T, int SLOTS>
__global__ __launch_bounds__(256, SWIFTK_MN_OCC) void modnorm_chunk_kernel(const T* __restrict__ y, int64_t ldy, float* __restrict__ x,
                                                            T* __restrict__ xc, int64_t ldc, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ mod,
                                                            int64_t ldmod, int64_t M, int d, int64_t rps, float eps, int nt_x,
                                                            bf16_t* __restrict__ x3 = nullptr, int64_t ld3 = 0, int64_t kv3 = 0) {
    const bool NT_X = nt_x & 1;
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int nc = d >> 3;
    const int64_t row0 = (int64_t)blockIdx.x * MN_ROWS + wv;
    const int64_t row_end = min((int64_t)(blockIdx.x + 1) * MN_ROWS, M);
    // P and Q of the chunk's (first) sample live in LDS, shared by the four waves: 8.4 KB per workgroup instead of 48
    // registers per lane, which is what lets three waves per SIMD keep two rows each in flight
    __shared__ __attribute__((aligned(16))) float sP[2048], sQ[2048];
    const int64_t blk_sample = ((int64_t)blockIdx.x * MN_ROWS) / rps;
    {
        const float* mrow = mod + blk_sample * ldmod;
        for (int c = threadIdx.x; c < nc; c += 256) {
            float g[8], bt[8], sc[8], sh[8], p[8], q[8];
            load8<float>(gamma + 8 * c, g);
            load8<float>(beta + 8 * c, bt);
            load8<float>(mrow + 8 * c, sc);
            load8<float>(mrow + d + 8 * c, sh);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                p[e] = g[e] * (1.0f + sc[e]);
                q[e] = bt[e] * (1.0f + sc[e]) + sh[e];
            }
            store8<float>(sP + 8 * c, p);
            store8<float>(sQ + 8 * c, q);
        }
    }
    __syncthreads();
    if (row0 >= row_end) return;
    raw8<T> ya[SLOTS], yb[SLOTS];
    float xa[SLOTS][8], xb[SLOTS][8];
    auto load_row = [&](int64_t row, raw8<T> (&yr)[SLOTS], float (&xr)[SLOTS][8]) {
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            const int c = lane + 64 * i;
            if (c < nc) {
                load_raw(y + row * ldy + 8 * c, yr[i]);
                if (NT_X) load8_nt(x + row * d + 8 * c, xr[i]); else load8<float>(x + row * d + 8 * c, xr[i]);
            }
        }
    };
    auto finish_row = [&](int64_t row, raw8<T> (&yr)[SLOTS], float (&xr)[SLOTS][8]) {
        float v[SLOTS][8];
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < SLOTS; ++i)
            if (lane + 64 * i < nc) {
                unpack_raw(yr[i], v[i]);
                sum += ((v[i][0] + v[i][1]) + (v[i][2] + v[i][3])) + ((v[i][4] + v[i][5]) + (v[i][6] + v[i][7]));
            }
        const float mean = wave_sum(sum) / (float)d;
        float sq = 0.f;
#pragma unroll
        for (int i = 0; i < SLOTS; ++i)
            if (lane + 64 * i < nc) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    v[i][e] -= mean;
                    sq += v[i][e] * v[i][e];
                }
            }
        const float rstd = rsqrtf(wave_sum(sq) / (float)d + eps);
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            const int c = lane + 64 * i;
            if (c < nc) {
                float P[8], Q[8];  // (the launcher takes this kernel only when no chunk straddles two samples)
                load8<float>(sP + 8 * c, P);
                load8<float>(sQ + 8 * c, Q);
#pragma unroll
                for (int e = 0; e < 8; ++e) xr[i][e] += (v[i][e] * rstd) * P[e] + Q[e];
                if (NT_X) store8_nt(x + row * d + 8 * c, xr[i]); else store8<float>(x + row * d + 8 * c, xr[i]);
                if (xc) store8<T>(xc + row * ldc + 8 * c, xr[i]);
                if (x3) {
                    // split engine (round 6): the row leaves as the NEXT GEMM's operand blocks [hi | lo | hi] as well -- bit for bit what
                    // swiftk_split3(order 0) makes of the fp32 row (hi = bf16(v), lo = bf16(v - hi)), without the pass that re-reads it
                    float lo[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) lo[e] = xr[i][e] - bf2f(f2bf(xr[i][e]));
                    bf16_t* r3 = x3 + row * ld3 + 8 * c;
                    store8<bf16_t>(r3, xr[i]);
                    store8<bf16_t>(r3 + kv3, lo);
                    store8<bf16_t>(r3 + 2 * kv3, xr[i]);
                }
            }
        }
        if (x3) {  // zero k-padding behind the three blocks (at most one 128-B k-tile row: 8 chunks)
            const int pad = (int)((ld3 - 3 * kv3) >> 3);
            if (lane < pad) *reinterpret_cast<uint4*>(x3 + row * ld3 + 3 * kv3 + 8 * lane) = make_uint4(0u, 0u, 0u, 0u);
        }
    };
    load_row(row0, ya, xa);
    for (int64_t row = row0; row < row_end; row += 8) {  // two rows per trip: the buffers swap roles without register moves
        if (row + 4 < row_end) load_row(row + 4, yb, xb);
        finish_row(row, ya, xa);
        if (row + 4 >= row_end) break;
        if (row + 8 < row_end) load_row(row + 8, ya, xa);
        finish_row(row + 4, yb, xb);
    }
}


// Pair form of the bf16 engine's residual stream (round 4): x is held as two bf16 tensors, hi = bf16(x) and
// lo = bf16(x - hi) (x = hi + lo to 2^-17 relative), so that hi IS the next GEMM's operand -- no separate operand copy.
// Bytes per element: y 2 + hi 2 + lo 2 in, hi 2 + lo 2 out = 10 (the fp32 stream + bf16 copy moved 14).  Same chunk
// scheme as modnorm_chunk_kernel: a workgroup owns MN_ROWS rows, P / Q folded once into LDS, two rows in flight per wave;
// the residual waits packed (8 registers per slot for hi and lo, as the fp32 form's 8).
__device__ __forceinline__ uint4 load_q(const bf16_t* p) { return *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ uint4 load_q_nt(const bf16_t* p) {
    typedef __attribute__((ext_vector_type(4))) uint32_t u4;
    const u4 a = __builtin_nontemporal_load(reinterpret_cast<const u4*>(p));
    return make_uint4(a[0], a[1], a[2], a[3]);
}
__device__ __forceinline__ void store_q_nt(bf16_t* p, const uint4& q) {
    typedef __attribute__((ext_vector_type(4))) uint32_t u4;
    __builtin_nontemporal_store(u4{q.x, q.y, q.z, q.w}, reinterpret_cast<u4*>(p));
}


// YF32: y arrives as TWO fp32 slabs (y and y + yslab, row stride ldy) whose sum is the branch output -- the split-K form of wo / w2
// at one or two units per step, where 96 output tiles cannot fill 256 CUs (forward.hip)
// YM = 2: the two slabs are bf16 (one unit per step: 10 instead of 14 bytes per element; each partial sum is rounded like y itself)
template <int SLOTS, bool LO8, int YM>
__global__ __launch_bounds__(256, (SLOTS == 3 && YM == 0) ? SWIFTK_MNP_OCC : ((SLOTS == 4 && YM != 0) ? 1 : 2)) void modnorm_pair_kernel(const void* __restrict__ y_, int64_t ldy, int64_t yslab,
                                                            bf16_t* __restrict__ xh, int64_t ldh, void* __restrict__ xl_,
                                                            int64_t ldl, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ mod,
                                                            int64_t ldmod, int64_t M, int d, int64_t rps, float eps, int nt) {
    constexpr bool YF32 = YM != 0;  // (the row's y is held as eight summed floats per slot)
    const bool NT = nt & 1;
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int nc = d >> 3;
    const int64_t row0 = (int64_t)blockIdx.x * MN_ROWS + wv;
    const int64_t row_end = min((int64_t)(blockIdx.x + 1) * MN_ROWS, M);
    __shared__ __attribute__((aligned(16))) float sP[2048], sQ[2048];
    const int64_t blk_sample = ((int64_t)blockIdx.x * MN_ROWS) / rps;
    {
        const float* mrow = mod + blk_sample * ldmod;
        for (int c = threadIdx.x; c < nc; c += 256) {
            float g[8], bt[8], sc[8], sh[8], p[8], q[8];
            load8<float>(gamma + 8 * c, g);
            load8<float>(beta + 8 * c, bt);
            load8<float>(mrow + 8 * c, sc);
            load8<float>(mrow + d + 8 * c, sh);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                p[e] = g[e] * (1.0f + sc[e]);
                q[e] = bt[e] * (1.0f + sc[e]) + sh[e];
            }
            store8<float>(sP + 8 * c, p);
            store8<float>(sQ + 8 * c, q);
        }
    }
    __syncthreads();
    if (row0 >= row_end) return;
    const bf16_t* y = static_cast<const bf16_t*>(y_);
    const float* yf = static_cast<const float*>(y_);
    bf16_t* xl = static_cast<bf16_t*>(xl_);   // bf16 low parts ...
    uint8_t* xl8 = static_cast<uint8_t*>(xl_);  // ... or one byte each (LO8)
    using LoT = typename std::conditional<LO8, uint2, uint4>::type;  // a slot's low parts: 8 bytes or 8 bf16
    using YT = typename std::conditional<YF32, raw8<float>, uint4>::type;  // a slot of y: 8 bf16, or the 8 summed floats
    struct Row { YT y[SLOTS]; uint4 h[SLOTS]; LoT l[SLOTS]; };
    Row ra, rb;
    auto load_row = [&](int64_t row, Row& r) {
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            const int c = lane + 64 * i;
            if (c < nc) {
                if constexpr (YM == 2) {
                    raw8<bf16_t> t0, t1;
                    t0.q = load_q(y + row * ldy + 8 * c);
                    t1.q = load_q(y + yslab + row * ldy + 8 * c);
                    float f0[8], f1[8];
                    unpack_raw(t0, f0);
                    unpack_raw(t1, f1);
                    r.y[i].a = make_float4(f0[0] + f1[0], f0[1] + f1[1], f0[2] + f1[2], f0[3] + f1[3]);
                    r.y[i].b = make_float4(f0[4] + f1[4], f0[5] + f1[5], f0[6] + f1[6], f0[7] + f1[7]);
                } else if constexpr (YF32) {
                    raw8<float> s0, s1;
                    load_raw(yf + row * ldy + 8 * c, s0);
                    load_raw(yf + yslab + row * ldy + 8 * c, s1);
                    r.y[i].a = make_float4(s0.a.x + s1.a.x, s0.a.y + s1.a.y, s0.a.z + s1.a.z, s0.a.w + s1.a.w);
                    r.y[i].b = make_float4(s0.b.x + s1.b.x, s0.b.y + s1.b.y, s0.b.z + s1.b.z, s0.b.w + s1.b.w);
                } else {
                    r.y[i] = NT ? load_q_nt(y + row * ldy + 8 * c) : load_q(y + row * ldy + 8 * c);
                }
                r.h[i] = load_q(xh + row * ldh + 8 * c);
                if constexpr (LO8) {
                    r.l[i] = *reinterpret_cast<const uint2*>(xl8 + row * ldl + 8 * c);
                } else {
                    r.l[i] = NT ? load_q_nt(xl + row * ldl + 8 * c) : load_q(xl + row * ldl + 8 * c);
                }
            }
        }
    };
    auto finish_row = [&](int64_t row, Row& r) {
        float v[SLOTS][8];
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < SLOTS; ++i)
            if (lane + 64 * i < nc) {
                if constexpr (YF32) {
                    unpack_raw(r.y[i], v[i]);
                } else {
                    raw8<bf16_t> t;
                    t.q = r.y[i];
                    unpack_raw(t, v[i]);
                }
                sum += ((v[i][0] + v[i][1]) + (v[i][2] + v[i][3])) + ((v[i][4] + v[i][5]) + (v[i][6] + v[i][7]));
            }
        const float mean = wave_sum(sum) / (float)d;
        float sq = 0.f;
#pragma unroll
        for (int i = 0; i < SLOTS; ++i)
            if (lane + 64 * i < nc) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    v[i][e] -= mean;
                    sq += v[i][e] * v[i][e];
                }
            }
        const float rstd = rsqrtf(wave_sum(sq) / (float)d + eps);
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            const int c = lane + 64 * i;
            if (c < nc) {
                float P[8], Q[8], hi[8], lo[8];
                load8<float>(sP + 8 * c, P);
                load8<float>(sQ + 8 * c, Q);
                raw8<bf16_t> t;
                t.q = r.h[i];
                unpack_raw(t, hi);
                if constexpr (LO8) {
                    const uint32_t hb[4] = {r.h[i].x, r.h[i].y, r.h[i].z, r.h[i].w};
                    const uint32_t lb[2] = {r.l[i].x, r.l[i].y};
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const uint32_t E = (hb[e >> 1] >> ((e & 1) ? 23 : 7)) & 0xFFu;
                        const uint32_t w = lb[e >> 2];
                        const float b = (float)((w >> (8 * (e & 3))) & 0xFFu);  // (selected as one v_cvt_f32_ubyteN)
                        lo[e] = lo8_value(b, E);
                    }
                } else {
                    const LoT lq = r.l[i];
                    t.q = make_uint4(lq.x, lq.y, reinterpret_cast<const uint32_t*>(&lq)[LO8 ? 0 : 2], reinterpret_cast<const uint32_t*>(&lq)[LO8 ? 1 : 3]);
                    unpack_raw(t, lo);
                }
                uint32_t oh[4], ol[4] = {0u, 0u, 0u, 0u};
                float xn[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) xn[e] = (hi[e] + lo[e]) + ((v[i][e] * rstd) * P[e] + Q[e]);
#pragma unroll
                for (int e2 = 0; e2 < 4; ++e2) {
                    const uint32_t ph = pack_bf16(xn[2 * e2], xn[2 * e2 + 1]);  // one v_cvt_pk_bf16_f32 per pair
                    oh[e2] = ph;
                    const float h0 = __uint_as_float(ph << 16), h1 = __uint_as_float(ph & 0xffff0000u);
                    if constexpr (LO8) {
                        ol[e2 >> 1] = lo8_insert(xn[2 * e2], h0, (ph >> 7) & 0xFFu, (2 * e2) & 3, ol[e2 >> 1]);
                        ol[e2 >> 1] = lo8_insert(xn[2 * e2 + 1], h1, (ph >> 23) & 0xFFu, (2 * e2 + 1) & 3, ol[e2 >> 1]);
                    } else {
                        ol[e2] = pack_bf16(xn[2 * e2] - h0, xn[2 * e2 + 1] - h1);
                    }
                }
                *reinterpret_cast<uint4*>(xh + row * ldh + 8 * c) = make_uint4(oh[0], oh[1], oh[2], oh[3]);
                if constexpr (LO8) {
                    *reinterpret_cast<uint2*>(xl8 + row * ldl + 8 * c) = make_uint2(ol[0], ol[1]);
                } else {
                    if (NT) store_q_nt(xl + row * ldl + 8 * c, make_uint4(ol[0], ol[1], ol[2], ol[3]));
                    else *reinterpret_cast<uint4*>(xl + row * ldl + 8 * c) = make_uint4(ol[0], ol[1], ol[2], ol[3]);
                }
            }
        }
    };
    load_row(row0, ra);
    for (int64_t row = row0; row < row_end; row += 8) {
        if (row + 4 < row_end) load_row(row + 4, rb);
        finish_row(row, ra);
        if (row + 4 >= row_end) break;
        if (row + 8 < row_end) load_row(row + 8, ra);
        finish_row(row + 4, rb);
    }
}

// Packed form of the pair kernel (8-bit low part, bf16 y, contiguous y / lo rows) for row widths that are not a multiple of
// 64 chunks: d = 1056 is 132 16-byte chunks = 2 x 64 + 4, so the row-per-wave form above issues every third instruction for 4
// of its 64 lanes -- a third of the VALU work and of the memory instructions of a kernel that is instruction- as much as
// byte-bound at 8 bytes per element.  Here a wave takes FOUR consecutive rows at a time and spreads their 4 NC chunks over its
// lanes without gaps (chunk q = 64 s + lane of the batch = row q / NC, column chunk q % NC: 9 slots instead of 12 for NC = 132,
// 10 instead of 12 for 160); which row(s) a slot holds and where the boundary lane sits are compile-time constants, so the row
// statistics are static selects plus one wave reduction per row and statistic, as before.  All of a batch's loads are issued up
// front (90 registers of packed data); y is unpacked again in each of the three passes (sum, centred squares, update) instead
// of being kept as 72 floats.  No second batch in flight: three waves per SIMD cover the latency.
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// Y2 (round 6, small batches): y arrives as two bf16 k-half slabs of the producing GEMM for the rows from `rows2` on (y1 = slab 1; rows
// below rows2 have slab 0 only): the halves are added in fp32 and rounded to bf16 once -- the value a whole-K tile would have
// rounded to, up to that one extra rounding -- and the kernel goes on as for one y
template <int NC, bool Y2 = false>
__global__ __launch_bounds__(256, SWIFTK_MNPK_OCC) void modnorm_pair_packed_kernel(const bf16_t* __restrict__ y, const bf16_t* xh, bf16_t* xh_out,
                                                                    int64_t ldh, uint8_t* __restrict__ xl, const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta, const float* __restrict__ mod,
                                                                    int64_t ldmod, int64_t M, int64_t rps, float eps, int nt,
                                                                    const bf16_t* __restrict__ y1 = nullptr, int64_t rows2 = 0,
                                                                    int tail_from = 0, int gm = 8, uint32_t chunk0 = 0) {
    constexpr int D = 8 * NC, NS = (4 * NC + 63) / 64;
    // (measured, 96 units: low part non-temporal 1.465 ms, plain 1.477; hi loads non-temporal 1.555 -- hi stays cached, it is the
    // next GEMM's operand; all forms of this kernel move their bytes at 4.5-4.9 TB/s, the rate a device copy reaches here)
    constexpr bool lo_nt = true;
    (void)nt;
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    __shared__ __attribute__((aligned(16))) float sP[D], sQ[D];
    // Y2: the two-slab chunks (the last ones) are dealt evenly among the others -- every R-th workgroup takes one -- instead of forming
    // the tail of the launch, where their two request phases would have nothing to hide behind
    // (32-bit arithmetic: a 64-bit division is ~100 instructions on this machine, and a workgroup's whole job is 16 rows)
    uint32_t chunk = blockIdx.x + chunk0;  // (chunk0: the launch covers the rows from 16 chunk0 on)
    if constexpr (Y2) {
        const uint32_t C = (uint32_t)(M / MN_ROWS), C2 = C - (uint32_t)(rows2 / MN_ROWS);
        if (C2 > 0 && C2 < C && chunk0 == 0) {
            const uint32_t R = C / C2, k = chunk / R;
            if (chunk - k * R == R - 1 && k < C2) chunk = (C - C2) + k;
            else chunk -= k < C2 ? k : C2;
        }
    }
    const int64_t blk_sample = Y2 ? (int64_t)((chunk * (uint32_t)MN_ROWS) / (uint32_t)rps) : ((int64_t)chunk * MN_ROWS) / rps;
    {
        const float* mrow = mod + blk_sample * ldmod;
        for (int c = threadIdx.x; c < NC; c += 256) {
            float g[8], bt[8], sc[8], sh[8], p[8], q[8];
            load8<float>(gamma + 8 * c, g);
            load8<float>(beta + 8 * c, bt);
            load8<float>(mrow + 8 * c, sc);
            load8<float>(mrow + D + 8 * c, sh);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                p[e] = g[e] * (1.0f + sc[e]);
                q[e] = bt[e] * (1.0f + sc[e]) + sh[e];
            }
            store8<float>(sP + 8 * c, p);
            store8<float>(sQ + 8 * c, q);
        }
    }
    __syncthreads();
    const int64_t r0 = (int64_t)chunk * MN_ROWS + 4 * wv;  // (the launcher guarantees M % 16 == 0)
    if (r0 >= M) return;
    const bf16_t* yb = y + r0 * D;
    uint8_t* lb = xl + r0 * D;
    const bf16_t* hb = xh + r0 * ldh;
    bf16_t* hbo = xh_out + r0 * ldh;  // (== hb in the inference engine; the training forward keeps the old hi: a saved activation)
    uint4 yq[NS], hq[NS];
    uint2 lq[NS];
    // slot s: row R0 for the lanes below BL, row R0 + 1 from BL on (BL >= 64: one row); the batch's last slot ends at lane VL
#define SWIFTK_SLOT(S_)                                                                                                     \
    constexpr int s = decltype(S_)::value;                                                                                  \
    constexpr int R0 = (64 * (s)) / NC, BL = (R0 + 1) * NC - 64 * (s), VL = 4 * NC - 64 * (s);                                \
    const bool up = BL < 64 && lane >= BL;           /* this lane's chunk belongs to row R0 + 1 */                          \
    const bool live = VL >= 64 || lane < VL;                                                                                \
    const int colc = lane + 64 * (s) - R0 * NC - (up ? NC : 0); /* column chunk inside the row */                           \
    const uint32_t hoff = (uint32_t)((R0 + (up ? 1 : 0)) * (int)ldh + 8 * colc)  /* (4 rows x ldh elements: fits 32 bits) */
    bool y_loaded = false;
    if constexpr (Y2) {
        // rows with two halves (wave-uniform: rows2 is a multiple of the 16-row chunk): both slabs' chunks are requested back to back and
        // added BEFORE the hi / lo requests go out -- the second slab's registers are free again by then (154 registers, three waves per
        // SIMD, as the one-y form).  Measured against everything requested up front (190 registers, two waves per SIMD): 60.0 against
        // 62.5 us at four units, 18.6 against 20.0 us at one (`profiles/r06zb_small_batch_tail_split.txt`)
        if (r0 >= rows2) {
            uint4 tq[NS];
            const bf16_t* yb1 = y1 + r0 * D;
            // the producing GEMM's tile of a chunk, in its walk's order (TileIter: groups of gm tile rows, column-major inside a group; 256 x 352
            // tiles = 44 chunks wide): slab 1 exists under tiles >= tail_from only (tail_from = 0: everywhere)
            const int ntm = (int)((M + 255) >> 8), grp_rows = gm * (NC / 44);
            static_for<0, NS>([&](auto S_) {
                SWIFTK_SLOT(S_);
                yq[s] = tq[s] = make_uint4(0u, 0u, 0u, 0u);
                if (live) {
                    yq[s] = load_q_nt(yb + 8 * (64 * s + lane));
                    const int tm = (int)((r0 + R0 + (up ? 1 : 0)) >> 8), grp = tm / gm, rows = min(gm, ntm - grp * gm);
                    const int tile = grp * grp_rows + (colc / 44) * rows + (tm - grp * gm);
                    if (tile >= tail_from) tq[s] = load_q_nt(yb1 + 8 * (64 * s + lane));
                }
            });
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                raw8<bf16_t> ta, tb;
                ta.q = yq[s];
                tb.q = tq[s];
                float va[8], vb[8];
                unpack_raw(ta, va);
                unpack_raw(tb, vb);
                yq[s] = make_uint4(pack_bf16(va[0] + vb[0], va[1] + vb[1]), pack_bf16(va[2] + vb[2], va[3] + vb[3]),
                                   pack_bf16(va[4] + vb[4], va[5] + vb[5]), pack_bf16(va[6] + vb[6], va[7] + vb[7]));
            }
            y_loaded = true;
        }
    }
    static_for<0, NS>([&](auto S_) {
        SWIFTK_SLOT(S_);
        if (!y_loaded) yq[s] = make_uint4(0u, 0u, 0u, 0u);
        hq[s] = make_uint4(0u, 0u, 0u, 0u);
        lq[s] = make_uint2(0u, 0u);
        if (live) {
            if (!y_loaded) yq[s] = load_q_nt(yb + 8 * (64 * s + lane));
            hq[s] = load_q(hb + hoff);
            if (lo_nt) {
                typedef __attribute__((ext_vector_type(2))) uint32_t u2;
                const u2 t = __builtin_nontemporal_load(reinterpret_cast<const u2*>(lb + 8 * (64 * s + lane)));
                lq[s] = make_uint2(t[0], t[1]);
            } else {
                lq[s] = *reinterpret_cast<const uint2*>(lb + 8 * (64 * s + lane));
            }
        }
    });
    auto unpack = [&](const uint4& q, float (&v)[8]) {
        raw8<bf16_t> t;
        t.q = q;
        unpack_raw(t, v);
    };
    // pass 1: row sums (a dead lane's zeros add nothing)
    float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    static_for<0, NS>([&](auto S_) {
        SWIFTK_SLOT(S_);
        float v[8];
        unpack(yq[s], v);
        const float p = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
        if constexpr (BL >= 64) {
            acc[R0] += p;
        } else {
            const float a = up ? 0.f : p;
            acc[R0] += a;
            acc[R0 + 1] += p - a;
        }
    });
    float mean[5];
#pragma unroll
    for (int r = 0; r < 4; ++r) mean[r] = wave_sum(acc[r]) * (1.0f / (float)D);
    mean[4] = 0.f;
    // (opaque: without it hipcc keeps the 72 unpacked floats of pass 1 alive for passes 2 and 3 -- 256 VGPRs and spills)
#pragma unroll
    for (int s = 0; s < NS; ++s) asm volatile("" : "+v"(yq[s].x), "+v"(yq[s].y), "+v"(yq[s].z), "+v"(yq[s].w));
    // pass 2: centred squares
#pragma unroll
    for (int r = 0; r < 5; ++r) acc[r] = 0.f;
    static_for<0, NS>([&](auto S_) {
        SWIFTK_SLOT(S_);
        float v[8];
        unpack(yq[s], v);
        const float m = (BL < 64 && up) ? mean[R0 + 1] : mean[R0];
        float p = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float c = v[e] - m;
            p += c * c;
        }
        p = live ? p : 0.f;  // (a dead lane's zeros minus the mean are not zero)
        if constexpr (BL >= 64) {
            acc[R0] += p;
        } else {
            const float a = up ? 0.f : p;
            acc[R0] += a;
            acc[R0 + 1] += p - a;
        }
    });
    float rstd[5];
#pragma unroll
    for (int r = 0; r < 4; ++r) rstd[r] = rsqrtf(wave_sum(acc[r]) * (1.0f / (float)D) + eps);
    rstd[4] = 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s) asm volatile("" : "+v"(yq[s].x), "+v"(yq[s].y), "+v"(yq[s].z), "+v"(yq[s].w));
    // pass 3: update and store
    static_for<0, NS>([&](auto S_) {
        SWIFTK_SLOT(S_);
        if (!live) return;
        float v[8], hi[8], P[8], Q[8];
        unpack(yq[s], v);
        unpack(hq[s], hi);
        load8<float>(sP + 8 * colc, P);
        load8<float>(sQ + 8 * colc, Q);
        const float m = (BL < 64 && up) ? mean[R0 + 1] : mean[R0];
        const float rs = (BL < 64 && up) ? rstd[R0 + 1] : rstd[R0];
        const uint32_t hw[4] = {hq[s].x, hq[s].y, hq[s].z, hq[s].w};
        const uint32_t lw[2] = {lq[s].x, lq[s].y};
        float xn[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const uint32_t E = (hw[e >> 1] >> ((e & 1) ? 23 : 7)) & 0xFFu;
            const float b = (float)((lw[e >> 2] >> (8 * (e & 3))) & 0xFFu);
            xn[e] = (hi[e] + lo8_value(b, E)) + (((v[e] - m) * rs) * P[e] + Q[e]);
        }
        uint32_t oh[4], ol[2] = {0u, 0u};
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) {
            const uint32_t ph = pack_bf16(xn[2 * e2], xn[2 * e2 + 1]);
            oh[e2] = ph;
            ol[e2 >> 1] = lo8_insert(xn[2 * e2], __uint_as_float(ph << 16), (ph >> 7) & 0xFFu, (2 * e2) & 3, ol[e2 >> 1]);
            ol[e2 >> 1] = lo8_insert(xn[2 * e2 + 1], __uint_as_float(ph & 0xffff0000u), (ph >> 23) & 0xFFu, (2 * e2 + 1) & 3, ol[e2 >> 1]);
        }
        *reinterpret_cast<uint4*>(hbo + hoff) = make_uint4(oh[0], oh[1], oh[2], oh[3]);
        if (lo_nt) {
            typedef __attribute__((ext_vector_type(2))) uint32_t u2;
            __builtin_nontemporal_store(u2{ol[0], ol[1]}, reinterpret_cast<u2*>(lb + 8 * (64 * s + lane)));
        } else {
            *reinterpret_cast<uint2*>(lb + 8 * (64 * s + lane)) = make_uint2(ol[0], ol[1]);
        }
    });
#undef SWIFTK_SLOT
}

// fp32 -> (hi, lo) bf16 pair, hi with zeroed k-padding columns [cols, ldh) (it is a GEMM operand), lo [rows, ldl]
__global__ __launch_bounds__(256) void split_pair_kernel(const float* __restrict__ src, int64_t lds, bf16_t* __restrict__ hi,
                                                         int64_t ldh, void* __restrict__ lo_, int64_t ldl, int64_t rows,
                                                         int64_t cols, int lo8) {
    bf16_t* lo = static_cast<bf16_t*>(lo_);
    const int64_t per = ldh >> 2, total = rows * per;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / per, c = i - r * per;
        if (4 * c >= cols) {
            *reinterpret_cast<uint2*>(hi + r * ldh + 4 * c) = make_uint2(0u, 0u);
            continue;
        }
        const float4 v = *reinterpret_cast<const float4*>(src + r * lds + 4 * c);
        const float f[4] = {v.x, v.y, v.z, v.w};
        bf16_t h[4], l[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            h[e] = f2bf(f[e]);
            l[e] = f2bf(f[e] - bf2f(h[e]));
        }
        *reinterpret_cast<uint2*>(hi + r * ldh + 4 * c) =
            make_uint2((uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16));
        if (lo8) {
            uint32_t b = 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) b = lo8_insert(f[e], bf2f(h[e]), ((uint32_t)h[e] >> 7) & 0xFFu, e, b);
            *reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(lo_) + r * ldl + 4 * c) = b;
        } else {
            *reinterpret_cast<uint2*>(lo + r * ldl + 4 * c) =
                make_uint2((uint32_t)l[0] | ((uint32_t)l[1] << 16), (uint32_t)l[2] | ((uint32_t)l[3] << 16));
        }
    }
}

// --------------------------------------------------------------------------------- patchify
// Thread per output element so that the GEMM operand is written fully coalesced; the strided reads hit L2
// (each 128-B input line is shared by 16 tokens x p2).
struct PatchArgs {
    const float* src[3];
    int c0[3];  // first channel of each source in the concatenated order
    int cn[3];
    float sc[3];
    const float* sc0;  // optional [B] per-sample factor on source 0 (EDM's c_in), on top of sc[0]; nullptr = none
    int B, H, W, p1, p2, C, gh, gw;
    int64_t lda;
};

template <typename T>
__global__ __launch_bounds__(256) void patchify_kernel(PatchArgs a, T* __restrict__ A) {
    const int64_t total = (int64_t)a.B * a.gh * a.gw * a.lda;
    const int F = a.p1 * a.p2 * a.C;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int f = (int)(i % a.lda);
        const int64_t tokg = i / a.lda;
        float val = 0.f;
        if (f < F) {
            const int c = f % a.C, pp = f / a.C;
            const int i1 = pp / a.p2, i2 = pp - i1 * a.p2;
            const int gx = (int)(tokg % a.gw);
            const int64_t t2 = tokg / a.gw;
            const int gy = (int)(t2 % a.gh);
            const int64_t b = t2 / a.gh;
            const int s = c >= a.c0[2] ? 2 : (c >= a.c0[1] ? 1 : 0);
            const int64_t off = ((b * a.cn[s] + (c - a.c0[s])) * a.H + (gy * a.p1 + i1)) * a.W + gx * a.p2 + i2;
            val = a.src[s][off] * a.sc[s];
            if (s == 0 && a.sc0) val *= a.sc0[b];
        }
        A[i] = elem<T>::from_f(val);
    }
}

// Tiled form: one block per (sample, grid row, 16 consecutive tokens).  The C x p1 x (16 p2) source pixels of those tokens
// are read as whole 128-B row segments (float4 per thread, channel scale applied) into an LDS tile, then every thread
// assembles 16-B chunks of the output rows ((p1 p2 c) order, c fastest) from it: coalesced on both sides, where the
// element-per-thread form above gathers one cache line per lane.
template <typename T>
__global__ __launch_bounds__(256) void patchify_tiled_kernel(PatchArgs a, T* __restrict__ A, int rs) {
    extern __shared__ __attribute__((aligned(16))) float ptile[];
    const int tid = threadIdx.x;
    const int gxb = blockIdx.x, gy = blockIdx.y, b = blockIdx.z;
    const int q4 = (16 * a.p2) >> 2;  // float4 per tile row
    const int nload = a.C * a.p1 * q4;
    for (int i = tid; i < nload; i += 256) {
        const int q = i % q4, r = i / q4;
        const int i1 = r % a.p1, c = r / a.p1;
        const int s = c >= a.c0[2] ? 2 : (c >= a.c0[1] ? 1 : 0);
        const float* src = a.src[s] + (((int64_t)b * a.cn[s] + (c - a.c0[s])) * a.H + (gy * a.p1 + i1)) * a.W + gxb * 16 * a.p2 + 4 * q;
        float4 v = *reinterpret_cast<const float4*>(src);
        const float sc = (s == 0 && a.sc0) ? a.sc[0] * a.sc0[b] : a.sc[s];
        v.x *= sc; v.y *= sc; v.z *= sc; v.w *= sc;
        *reinterpret_cast<float4*>(ptile + r * rs + 4 * q) = v;
    }
    __syncthreads();
    const int F = a.p1 * a.p2 * a.C;
    const int cpr = (int)(a.lda >> 3);  // 8-element chunks per output row
    const int64_t tok0 = ((int64_t)b * a.gh + gy) * a.gw + gxb * 16;
    for (int i = tid; i < 16 * cpr; i += 256) {
        const int tk = i / cpr, fc = i - tk * cpr;
        float v[8];
        int f = 8 * fc;
        int pp = f / a.C, c = f - pp * a.C;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float val = 0.f;
            if (f < F) {
                const int i1 = pp / a.p2, i2 = pp - i1 * a.p2;
                val = ptile[(c * a.p1 + i1) * rs + tk * a.p2 + i2];
            }
            v[e] = val;
            ++f;
            if (++c == a.C) { c = 0; ++pp; }
        }
        store8<T>(A + (tok0 + tk) * a.lda + 8 * fc, v);
    }
}

// --------------------------------------------------------------------------------- un-patchify (+ sampler affine)
__global__ __launch_bounds__(256) void unpatchify_kernel(const float* __restrict__ tok, int64_t ldt,
                                                         const float* __restrict__ xt, const float* __restrict__ alpha,
                                                         const float* __restrict__ beta, float* __restrict__ out, int B,
                                                         int C, int H, int W, int p1, int p2) {
    const int64_t total = (int64_t)B * C * H * W;
    const int gw = W / p2, gh = H / p1;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int xw = (int)(i % W);
        int64_t r = i / W;
        const int yh = (int)(r % H);
        r /= H;
        const int c = (int)(r % C);
        const int64_t b = r / C;
        const int gy = yh / p1, i1 = yh - gy * p1, gx = xw / p2, i2 = xw - gx * p2;
        const float f = tok[(b * gh * gw + (int64_t)gy * gw + gx) * ldt + (c * p1 + i1) * p2 + i2];
        const float bb = beta ? beta[b] : 1.0f;
        float o = bb * f;
        if (xt) o = (alpha ? alpha[b] : 0.0f) * xt[i] + o;
        out[i] = o;
    }
}

// 2 x 2 patches (every shipped 1.4-degree config), W % 4 == 0, 16-B aligned rows: a thread produces four consecutive
// output pixels of one (sample, channel, image row) = the (i1, 0..1) pairs of two neighbouring tokens -- two 8-B reads, one
// 16-B read of x_t, one 16-B write instead of four 4-byte accesses each
__global__ __launch_bounds__(256) void unpatchify4_kernel(const float* __restrict__ tok, int64_t ldt,
                                                          const float* __restrict__ xt, const float* __restrict__ alpha,
                                                          const float* __restrict__ beta, float* __restrict__ out, int B,
                                                          int C, int H, int W) {
    const int W4 = W >> 2, gw = W >> 1, gh = H >> 1;
    const int64_t total = (int64_t)B * C * H * W4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int x4 = (int)(i % W4);
        int64_t r = i / W4;
        const int yh = (int)(r % H);
        r /= H;
        const int c = (int)(r % C);
        const int64_t b = r / C;
        const int gy = yh >> 1, i1 = yh & 1;
        const float* t0 = tok + (b * gh * gw + (int64_t)gy * gw + 2 * x4) * ldt + (c * 2 + i1) * 2;
        const float2 f0 = *reinterpret_cast<const float2*>(t0);
        const float2 f1 = *reinterpret_cast<const float2*>(t0 + ldt);
        const float bb = beta ? beta[b] : 1.0f;
        float4 o = make_float4(bb * f0.x, bb * f0.y, bb * f1.x, bb * f1.y);
        if (xt) {
            const float aa = alpha ? alpha[b] : 0.0f;
            const float4 x = *reinterpret_cast<const float4*>(xt + 4 * i);
            o.x = aa * x.x + o.x; o.y = aa * x.y + o.y; o.z = aa * x.z + o.z; o.w = aa * x.w + o.w;  // same operation order
        }
        *reinterpret_cast<float4*>(out + 4 * i) = o;
    }
}

// --------------------------------------------------------------------------------- time embedding
__global__ void temb_kernel(const float* __restrict__ t, const float* __restrict__ aux, const float* __restrict__ freqs,
                            const float* __restrict__ aux_w, const float* __restrict__ aux_b, float* __restrict__ emb,
                            int B, int d, int aux_dim, float tw) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * d) return;
    const int b = i / d, k = i - b * d, half = d >> 1;
    float v = 0.f;
    if (k < 2 * half) {
        const float arg = (t[b] * tw) * freqs[k < half ? k : k - half];
        v = k < half ? sinf(arg) : cosf(arg);
    }
    if (aux && aux_w) {
        const float s = sqrtf((float)aux_dim);
        float acc = 0.f;
        for (int j = 0; j < aux_dim; ++j) acc += (aux[b * aux_dim + j] * s) * aux_w[k * aux_dim + j];
        v += acc + aux_b[k];
    }
    emb[i] = v;
}

// --------------------------------------------------------------------------------- per-unit checksum
// Order-fixed fp64 sum of every unit's [n] fp32 values: PARTS blocks per unit write partials, block 0..B-1 of the second
// launch adds them in index order -- the same bits for the same unit whatever rank or batch slot it ran in.
constexpr int CK_PARTS = 32;
__global__ __launch_bounds__(256) void checksum_part_kernel(const float* __restrict__ x, double* __restrict__ part, int64_t n) {
    __shared__ double red[256];
    const int u = blockIdx.y, p = blockIdx.x;
    const int64_t n4 = n >> 2, per = (n4 + CK_PARTS - 1) / CK_PARTS;
    const int64_t lo = p * per, hi = min(n4, lo + per);
    const float4* src = reinterpret_cast<const float4*>(x + (int64_t)u * n);
    double acc = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        const float4 v = src[i];
        acc += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[u * CK_PARTS + p] = red[0];
}
__global__ void checksum_final_kernel(const double* __restrict__ part, double* __restrict__ out, int B) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= B) return;
    double s = 0.0;
    for (int p = 0; p < CK_PARTS; ++p) s += part[u * CK_PARTS + p];
    out[u] = s;
}

// --------------------------------------------------------------------------------- small-batch linear, x in LDS
// The 24 modulation Linears as one [50688, 1056] matrix dominate this op: every weight row is read once from HBM, but
// with one wave per output feature the 8 x-rows were re-read from L1/L2 by each of the 50k waves (8x the weight bytes).
// Here a block stages its x rows in LDS once and its four waves walk output features against that copy.
template <int BB>
__global__ __launch_bounds__(256) void linear_small_lds_kernel(const float* __restrict__ x, int64_t ldx,
                                                               const float* __restrict__ W, int64_t ldw,
                                                               const float* __restrict__ bias, float* __restrict__ out,
                                                               int64_t ldo, int B, int N, int K, int act) {
    extern __shared__ __attribute__((aligned(16))) float xs[];  // [BB][K]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int k4 = K >> 2;
    for (int b0 = 0; b0 < B; b0 += BB) {
        const int nb = min(BB, B - b0);
        __syncthreads();
        for (int i = threadIdx.x; i < nb * k4; i += 256) {
            const int j = i / k4, c = i - j * k4;
            *reinterpret_cast<float4*>(xs + j * K + 4 * c) = *reinterpret_cast<const float4*>(x + (int64_t)(b0 + j) * ldx + 4 * c);
        }
        __syncthreads();
        if (k4 <= 5 * 64) {
            // a weight row is at most five 16-B loads per lane: the NEXT row's loads are issued before this row's cross-lane sums,
            // and only the live batch rows are summed (one unit per step: seven of eight reductions were of zeros -- the kernel
            // walked the 214-MB modulation matrix at 2.7 TB/s)
            const int n0 = blockIdx.x * 4 + wv, dn = gridDim.x * 4;
            float4 w[5];
            auto fetch = [&](int n, float4 (&r)[5]) {
#pragma unroll
                for (int u = 0; u < 5; ++u) {
                    const int c = lane + 64 * u;
                    r[u] = (n < N && c < k4) ? *reinterpret_cast<const float4*>(W + (int64_t)n * ldw + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            };
            fetch(n0, w);
            for (int n = n0; n < N; n += dn) {
                float acc[BB];
#pragma unroll
                for (int j = 0; j < BB; ++j) acc[j] = 0.f;
#pragma unroll
                for (int u = 0; u < 5; ++u) {
                    const int c = lane + 64 * u;
                    if (c < k4) {
#pragma unroll
                        for (int j = 0; j < BB; ++j) {
                            if (j < nb) {
                                const float4 xv = *reinterpret_cast<const float4*>(xs + j * K + 4 * c);
                                acc[j] += (w[u].x * xv.x + w[u].y * xv.y) + (w[u].z * xv.z + w[u].w * xv.w);
                            }
                        }
                    }
                }
                fetch(n + dn, w);
#pragma unroll
                for (int j = 0; j < BB; ++j) {
                    if (j < nb) {  // (block-uniform)
                        const float s = wave_sum(acc[j]);
                        if (lane == 0) {
                            float v = s + (bias ? bias[n] : 0.f);
                            if (act == 1) v = v / (1.0f + expf(-v));
                            out[(int64_t)(b0 + j) * ldo + n] = v;
                        }
                    }
                }
            }
            continue;
        }
        for (int n = blockIdx.x * 4 + wv; n < N; n += gridDim.x * 4) {
            float acc[BB];
#pragma unroll
            for (int j = 0; j < BB; ++j) acc[j] = 0.f;
            for (int c0 = 0; c0 < k4; c0 += 5 * 64) {  // five 16-B loads of the weight row in flight per lane
                float4 w[5];
#pragma unroll
                for (int u = 0; u < 5; ++u) {
                    const int c = c0 + lane + 64 * u;
                    w[u] = c < k4 ? *reinterpret_cast<const float4*>(W + (int64_t)n * ldw + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int u = 0; u < 5; ++u) {
                    const int c = c0 + lane + 64 * u;
                    if (c < k4) {
#pragma unroll
                        for (int j = 0; j < BB; ++j) {
                            if (j < nb) {
                                const float4 xv = *reinterpret_cast<const float4*>(xs + j * K + 4 * c);
                                acc[j] += (w[u].x * xv.x + w[u].y * xv.y) + (w[u].z * xv.z + w[u].w * xv.w);
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < BB; ++j) {
                const float s = wave_sum(acc[j]);
                if (lane == 0 && j < nb) {
                    float v = s + (bias ? bias[n] : 0.f);
                    if (act == 1) v = v / (1.0f + expf(-v));
                    out[(int64_t)(b0 + j) * ldo + n] = v;
                }
            }
        }
    }
}

// --------------------------------------------------------------------------------- small-batch linear
// One wave per output feature n, lanes stride over K in float4; x rows are tiny and stay in L1/L2.
template <int BB>
__global__ __launch_bounds__(256) void linear_small_kernel(const float* __restrict__ x, int64_t ldx,
                                                           const float* __restrict__ W, int64_t ldw,
                                                           const float* __restrict__ bias, float* __restrict__ out,
                                                           int64_t ldo, int B, int N, int K, int act) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const int k4 = K >> 2;
    for (int b0 = 0; b0 < B; b0 += BB) {
        float acc[BB];
#pragma unroll
        for (int j = 0; j < BB; ++j) acc[j] = 0.f;
        for (int c = lane; c < k4; c += 64) {
            const float4 w = *reinterpret_cast<const float4*>(W + (int64_t)n * ldw + 4 * c);
#pragma unroll
            for (int j = 0; j < BB; ++j) {
                if (b0 + j < B) {
                    const float4 xv = *reinterpret_cast<const float4*>(x + (int64_t)(b0 + j) * ldx + 4 * c);
                    acc[j] += (w.x * xv.x + w.y * xv.y) + (w.z * xv.z + w.w * xv.w);
                }
            }
        }
        for (int k = (k4 << 2) + lane; k < K; k += 64)  // K % 4 tail
#pragma unroll
            for (int j = 0; j < BB; ++j)
                if (b0 + j < B) acc[j] += W[(int64_t)n * ldw + k] * x[(int64_t)(b0 + j) * ldx + k];
#pragma unroll
        for (int j = 0; j < BB; ++j) {
            const float s = wave_sum(acc[j]);
            if (lane == 0 && b0 + j < B) {
                float v = s + (bias ? bias[n] : 0.f);
                if (act == 1) v = v / (1.0f + expf(-v));
                out[(int64_t)(b0 + j) * ldo + n] = v;
            }
        }
    }
}

// --------------------------------------------------------------------------------- rollout update
__global__ __launch_bounds__(256) void rollout_update_kernel(float* __restrict__ xstd, const float* __restrict__ y,
                                                             float* __restrict__ phys, const float* __restrict__ mx,
                                                             const float* __restrict__ sx, const float* __restrict__ st,
                                                             int C, int64_t hw4, int64_t total4) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int c = (int)((i / hw4) % C);
        const float m = mx[c], s = sx[c];
        const float4 yv = reinterpret_cast<const float4*>(y)[i];
        float4 p, q;
        if (!st) {  // non-residual dataset (generate.py:132-136): the network output IS the next standardised state
#pragma clang fp contract(off)  // two roundings, as the reference's `v * s + m`: no fused multiply-add
            p.x = yv.x * s + m; p.y = yv.y * s + m; p.z = yv.z * s + m; p.w = yv.w * s + m;
            if (phys) reinterpret_cast<float4*>(phys)[i] = p;
            reinterpret_cast<float4*>(xstd)[i] = yv;
            continue;
        }
        const float t = st[c];
        const float4 xv = reinterpret_cast<const float4*>(xstd)[i];
        p.x = (xv.x * s + m) + yv.x * t; p.y = (xv.y * s + m) + yv.y * t;
        p.z = (xv.z * s + m) + yv.z * t; p.w = (xv.w * s + m) + yv.w * t;
        q.x = (p.x - m) / s; q.y = (p.y - m) / s; q.z = (p.z - m) / s; q.w = (p.w - m) / s;
        // s == 0 marks a channel whose STANDARDISED value the dataset forces to zero (zero_field, data/era5.py:135-149:
        // sea_surface_temperature): the old state contributes nothing (x * 0 + m with m = 0), the residual still lands in the
        // physical output when its scale t is non-zero (--interval 24), and the next standardised state is 0
        if (s == 0.f) q = make_float4(0.f, 0.f, 0.f, 0.f);
        if (phys) reinterpret_cast<float4*>(phys)[i] = p;
        reinterpret_cast<float4*>(xstd)[i] = q;
    }
}

// (no __restrict__: out may be x or y -- every thread reads the elements it writes before it writes them)
__global__ __launch_bounds__(256) void axpby_kernel(float* out, float a, const float* x, float b, const float* y, int64_t n4,
                                                    int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 xv = reinterpret_cast<const float4*>(x)[i];
        const float4 yv = reinterpret_cast<const float4*>(y)[i];
        reinterpret_cast<float4*>(out)[i] = make_float4(a * xv.x + b * yv.x, a * xv.y + b * yv.y, a * xv.z + b * yv.z,
                                                        a * xv.w + b * yv.w);
    }
    if (blockIdx.x == 0)
        for (int64_t i = 4 * n4 + threadIdx.x; i < n; i += 256) out[i] = a * x[i] + b * y[i];
}

template <typename T>
__global__ __launch_bounds__(256) void cast_pad_kernel(const float* __restrict__ src, int64_t lds, T* __restrict__ dst,
                                                       int64_t ldd, int64_t rows, int64_t cols) {
    const int64_t total = rows * ldd;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / ldd, c = i - r * ldd;
        dst[i] = elem<T>::from_f(c < cols ? src[r * lds + c] : 0.f);
    }
}

// fp32 -> three bf16 column blocks: hi = bf16(v), lo = bf16(v - hi) (v = hi + lo to 2^-17 relative).  order 0 (activations):
// [hi | lo | hi], order 1 (weights): [hi | hi | lo], so that the ordinary bf16 GEMM over K' = 3 cols computes
// hi hi' + lo hi' + hi lo' with fp32 accumulation (the lo lo' term, 2^-18, is dropped); columns [3 cols, ldd) zero.
__global__ __launch_bounds__(256) void split3_kernel(const float* __restrict__ src, int64_t lds, bf16_t* __restrict__ dst,
                                                     int64_t ldd, int64_t rows, int64_t cols, int order) {
    const int64_t c4 = cols >> 2, p4 = (ldd - 3 * cols) >> 2, per = c4 + p4, total = rows * per;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / per, c = i - r * per;
        bf16_t* d = dst + r * ldd;
        if (c >= c4) {  // zero padding behind the three blocks
            *reinterpret_cast<uint2*>(d + 3 * cols + 4 * (c - c4)) = make_uint2(0u, 0u);
            continue;
        }
        const float4 v = *reinterpret_cast<const float4*>(src + r * lds + 4 * c);
        const float f[4] = {v.x, v.y, v.z, v.w};
        bf16_t hi[4], lo[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            hi[e] = f2bf(f[e]);
            lo[e] = f2bf(f[e] - bf2f(hi[e]));
        }
        const uint2 H = make_uint2((uint32_t)hi[0] | ((uint32_t)hi[1] << 16), (uint32_t)hi[2] | ((uint32_t)hi[3] << 16));
        const uint2 Lo = make_uint2((uint32_t)lo[0] | ((uint32_t)lo[1] << 16), (uint32_t)lo[2] | ((uint32_t)lo[3] << 16));
        *reinterpret_cast<uint2*>(d + 4 * c) = H;
        *reinterpret_cast<uint2*>(d + cols + 4 * c) = order == 0 ? Lo : H;
        *reinterpret_cast<uint2*>(d + 2 * cols + 4 * c) = order == 0 ? H : Lo;
    }
}

// --------------------------------------------------------------------------------- latent noise
// Counter-based N(0, 1) stream keyed by (unit seed, lead step, element): Philox4x32-10 (Salmon et al., SC'11; the
// Random123 constants) with key = the unit's 64-bit seed and counter = (element / 4, 0, step lo, step hi); the four 32-bit
// outputs feed two Box-Muller pairs.  A unit's noise therefore depends on nothing but (seed, step, element) -- not on the
// rank, the batch it sits in or the order of launches -- and the whole draw is one launch that a captured step can hold
// (the step number is read from device memory).  Replaces the latents of generating/factory.py:52-56 for production
// rollouts (generate.py:83 seeds a torch generator per member and consumes it in batch order).
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c[0]), l0 = 0xD2511F53u * c[0];
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c[2]), l1 = 0xCD9E8D57u * c[2];
        const uint32_t n0 = h1 ^ c[1] ^ k0, n2 = h0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = l1; c[2] = n2; c[3] = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

__global__ __launch_bounds__(256) void unit_noise_kernel(float* __restrict__ out, const int64_t* __restrict__ seeds,
                                                         const int64_t* __restrict__ step_dev, int64_t step_add, int64_t n4,
                                                         int mode) {
    const int b = blockIdx.y;
    const uint64_t seed = (uint64_t)seeds[b];
    const uint64_t step = (uint64_t)((step_dev ? *step_dev : 0) + step_add);
    float* o = out + (int64_t)b * n4 * 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        uint32_t c[4] = {(uint32_t)i, (uint32_t)((uint64_t)i >> 32), (uint32_t)step, (uint32_t)(step >> 32)};
        philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
        float4 z;
        if (mode == 1) {  // raw generator output (bit-exact check of the integer part against the oracle)
            z = make_float4(__uint_as_float(c[0]), __uint_as_float(c[1]), __uint_as_float(c[2]), __uint_as_float(c[3]));
        } else {
            // 24-bit uniforms strictly inside (0, 1): (k + 0.5) 2^-24 is exact in fp32
            const float u0 = ((float)(c[0] >> 8) + 0.5f) * 0x1p-24f, u1 = ((float)(c[1] >> 8) + 0.5f) * 0x1p-24f;
            const float u2 = ((float)(c[2] >> 8) + 0.5f) * 0x1p-24f, u3 = ((float)(c[3] >> 8) + 0.5f) * 0x1p-24f;
            const float ra = sqrtf(-2.0f * logf(u0)), rb = sqrtf(-2.0f * logf(u2));
            float sa, ca, sb, cb;
            sincospif(2.0f * u1, &sa, &ca);
            sincospif(2.0f * u3, &sb, &cb);
            z = make_float4(ra * ca, ra * sa, rb * cb, rb * sb);
        }
        *reinterpret_cast<float4*>(o + 4 * i) = z;
    }
}

__global__ void counter_add_kernel(int64_t* p, int64_t v) { *p += v; }

inline int grid_for(int64_t work_items, int per_block = 256, int cap = 256 * 16) {
    int64_t g = (work_items + per_block - 1) / per_block;
    if (g < 1) g = 1;
    return (int)(g > cap ? cap : g);
}


// y_slab == 0: y is bf16 [M, ldy]; y_slab > 0: y is the sum of two fp32 slabs [M, ldy] that many elements apart
static int modnorm_pair_impl(const void* y, int64_t ldy, int64_t y_slab, void* x_hi, int64_t ldh, void* x_lo, int64_t ldl,
                             int lo_bits, const float* gamma, const float* beta, const float* mod, int64_t ldmod, int64_t M, int d,
                             int64_t rows_per_sample, float eps, void* stream, void* x_hi_out = nullptr, bool slab_bf16 = false) {
    if (!y || !x_hi || !x_lo || !gamma || !beta || !mod || M <= 0 || d <= 0 || rows_per_sample <= 0) return SWIFTK_EINVAL;
    if (lo_bits != 16 && lo_bits != 8) return SWIFTK_EINVAL;
    if (d % 8 || d > 2048 || rows_per_sample % MN_ROWS) return SWIFTK_ESHAPE;
    if (ldy < d || ldh < d || ldl < d) return SWIFTK_ESHAPE;
    const int lb = lo_bits / 8, ys = (y_slab && !slab_bf16) ? 4 : 2;
    if (((uintptr_t)y & 15) || (ldy * ys) % 16 || ((uintptr_t)x_hi & 15) || (ldh * 2) % 16 || ((uintptr_t)x_lo & (8 * lb - 1)) ||
        (ldl * lb) % (8 * lb) || ((uintptr_t)gamma & 15) || ((uintptr_t)beta & 15) || ((uintptr_t)mod & 15) || (ldmod % 4))
        return SWIFTK_EALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int cgrid = (int)((M + MN_ROWS - 1) / MN_ROWS);
    // row widths of 132 / 160 chunks (d = 1056 / 1280) with the 8-bit low part and contiguous y / lo rows: the packed form
    const bool separate_out = x_hi_out && x_hi_out != x_hi;
    if (separate_out && (((uintptr_t)x_hi_out & 15))) return SWIFTK_EALIGN;
    if (!y_slab && lo_bits == 8 && ldy == d && ldl == d && M % MN_ROWS == 0 && ((g_modnorm_nt & 4) == 0 || separate_out) &&
        (d == 1056 || d == 1280)) {
        bf16_t* ho = static_cast<bf16_t*>(separate_out ? x_hi_out : x_hi);
        if (d == 1056)
            hipLaunchKernelGGL((modnorm_pair_packed_kernel<132>), dim3(cgrid), dim3(256), 0, st, static_cast<const bf16_t*>(y),
                               static_cast<const bf16_t*>(x_hi), ho, ldh, static_cast<uint8_t*>(x_lo), gamma, beta, mod, ldmod, M,
                               rows_per_sample, eps, g_modnorm_nt);
        else
            hipLaunchKernelGGL((modnorm_pair_packed_kernel<160>), dim3(cgrid), dim3(256), 0, st, static_cast<const bf16_t*>(y),
                               static_cast<const bf16_t*>(x_hi), ho, ldh, static_cast<uint8_t*>(x_lo), gamma, beta, mod, ldmod, M,
                               rows_per_sample, eps, g_modnorm_nt);
        SWIFTK_CHECK_LAUNCH();
        return 0;
    }
    if (separate_out) return SWIFTK_ESHAPE;  // the out-of-place hi exists in the packed kernel only (d = 1056 / 1280, 8-bit low part)
#define SWIFTK_MNP(SL, L8, YF)                                                                                                  \
    hipLaunchKernelGGL((modnorm_pair_kernel<SL, L8, YF>), dim3(cgrid), dim3(256), 0, st, y, ldy, y_slab,                          \
                       static_cast<bf16_t*>(x_hi), ldh, x_lo, ldl, gamma, beta, mod, ldmod, M, d, rows_per_sample, eps, g_modnorm_nt)
#define SWIFTK_MNP2(SL)                                                                   \
    do {                                                                                   \
        if (y_slab && slab_bf16) { if (lo_bits == 8) SWIFTK_MNP(SL, true, 2); else SWIFTK_MNP(SL, false, 2); }   \
        else if (y_slab) { if (lo_bits == 8) SWIFTK_MNP(SL, true, 1); else SWIFTK_MNP(SL, false, 1); }   \
        else { if (lo_bits == 8) SWIFTK_MNP(SL, true, 0); else SWIFTK_MNP(SL, false, 0); }        \
    } while (0)
    if (d <= 3 * 512) SWIFTK_MNP2(3); else SWIFTK_MNP2(4);
#undef SWIFTK_MNP2
#undef SWIFTK_MNP
    SWIFTK_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int swiftk_modnorm_residual(const void* y, int64_t ldy, float* x, void* xcopy, int64_t ldc, const float* gamma,
                                       const float* beta, const float* mod, int64_t ldmod, int64_t M, int d,
                                       int64_t rows_per_sample, float eps, int dtype, void* stream) {
    if (!y || !x || !gamma || !beta || !mod || M <= 0 || d <= 0 || rows_per_sample <= 0) return SWIFTK_EINVAL;
    if (d % 8 || d > 2048) return SWIFTK_ESHAPE;
    const int es = dtype == SWIFTK_BF16 ? 2 : 4;
    if (((uintptr_t)y & 15) || (ldy * es) % 16 || ((uintptr_t)x & 15) || ((uintptr_t)gamma & 15) || ((uintptr_t)beta & 15) ||
        ((uintptr_t)mod & 15) || (ldmod % 4) || (xcopy && (((uintptr_t)xcopy & 15) || (ldc * es) % 16)))
        return SWIFTK_EALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int grid = grid_for(M, 4, 1 << 20);  // one row per wave (a capped, looping grid measured 6 % slower)
    const bool small = d <= 3 * 512;  // three 8-channel slots per lane cover d <= 1536 with fewer registers
    const int cgrid = (int)((M + MN_ROWS - 1) / MN_ROWS);
#define SWIFTK_MODNORM(TT, SL)                                                                                             \
    if ((g_modnorm_nt & 2) && rows_per_sample % MN_ROWS == 0)                                                              \
        hipLaunchKernelGGL((modnorm_chunk_kernel<TT, SL>), dim3(cgrid), dim3(256), 0, st, static_cast<const TT*>(y), ldy, x, \
                           static_cast<TT*>(xcopy), ldc, gamma, beta, mod, ldmod, M, d, rows_per_sample, eps, g_modnorm_nt); \
    else                                                                                                                   \
        hipLaunchKernelGGL((modnorm_kernel<TT, SL>), dim3(grid), dim3(256), 0, st, static_cast<const TT*>(y), ldy, x,        \
                           static_cast<TT*>(xcopy), ldc, gamma, beta, mod, ldmod, M, d, rows_per_sample, eps, g_modnorm_nt & 1)
    if (dtype == SWIFTK_BF16) {
        if (small) { SWIFTK_MODNORM(bf16_t, 3); } else { SWIFTK_MODNORM(bf16_t, 4); }
    } else if (dtype == SWIFTK_F32) {
        if (small) { SWIFTK_MODNORM(float, 3); } else { SWIFTK_MODNORM(float, 4); }
    } else {
        return SWIFTK_EINVAL;
    }
#undef SWIFTK_MODNORM
    SWIFTK_CHECK_LAUNCH();
    return 0;
}

int g_x3_normsplit = 1;  // tuning key 26: split engine, the fp32 ModulatedNorm writes the next GEMM's (hi, lo, hi) operand blocks itself

extern "C" int swiftk_modnorm_residual_split3(const float* y, int64_t ldy, float* x, float* xcopy, int64_t ldc, void* x3, int64_t ld3,
                                              const float* gamma, const float* beta, const float* mod, int64_t ldmod, int64_t M, int d,
                                              int64_t rows_per_sample, float eps, void* stream) {
    if (!y || !x || !x3 || !gamma || !beta || !mod || M <= 0 || d <= 0 || rows_per_sample <= 0) return SWIFTK_EINVAL;
    // the chunked kernel only (whole 16-row chunks inside one sample); anything else: swiftk_modnorm_residual + swiftk_split3
    if (d % 8 || d > 2048 || rows_per_sample % MN_ROWS || !(g_modnorm_nt & 2) || ld3 < 3 * (int64_t)d || (ld3 - 3 * (int64_t)d) > 64 * 8 ||
        (ld3 - 3 * (int64_t)d) % 8)
        return SWIFTK_ESHAPE;
    if (((uintptr_t)y & 15) || (ldy * 4) % 16 || ((uintptr_t)x & 15) || ((uintptr_t)gamma & 15) || ((uintptr_t)beta & 15) || ((uintptr_t)mod & 15) ||
        (ldmod % 4) || (xcopy && (((uintptr_t)xcopy & 15) || (ldc * 4) % 16)) || ((uintptr_t)x3 & 15) || (ld3 * 2) % 16)
        return SWIFTK_EALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int cgrid = (int)((M + MN_ROWS - 1) / MN_ROWS);
    if (d <= 3 * 512)
        hipLaunchKernelGGL((modnorm_chunk_kernel<float, 3>), dim3(cgrid), dim3(256), 0, st, y, ldy, x, xcopy, ldc, gamma, beta, mod, ldmod, M, d,
                           rows_per_sample, eps, g_modnorm_nt, static_cast<bf16_t*>(x3), ld3, (int64_t)d);
    else
        hipLaunchKernelGGL((modnorm_chunk_kernel<float, 4>), dim3(cgrid), dim3(256), 0, st, y, ldy, x, xcopy, ldc, gamma, beta, mod, ldmod, M, d,
                           rows_per_sample, eps, g_modnorm_nt, static_cast<bf16_t*>(x3), ld3, (int64_t)d);
    SWIFTK_CHECK_LAUNCH();
    return 0;
}

extern "C" int swiftk_modnorm_residual_pair(const void* y, int64_t ldy, void* x_hi, int64_t ldh, void* x_lo, int64_t ldl,
                                            int lo_bits, const float* gamma, const float* beta, const float* mod, int64_t ldmod,
                                            int64_t M, int d, int64_t rows_per_sample, float eps, void* stream) {
    return modnorm_pair_impl(y, ldy, 0, x_hi, ldh, x_lo, ldl, lo_bits, gamma, beta, mod, ldmod, M, d, rows_per_sample, eps, stream);
}

extern "C" int swiftk_modnorm_residual_pair_to(const void* y, int64_t ldy, const void* x_hi_in, void* x_hi_out, int64_t ldh, void* x_lo,
                                               int64_t ldl, int lo_bits, const float* gamma, const float* beta, const float* mod,
                                               int64_t ldmod, int64_t M, int d, int64_t rows_per_sample, float eps, void* stream) {
    if (!x_hi_out) return SWIFTK_EINVAL;
    return modnorm_pair_impl(y, ldy, 0, const_cast<void*>(x_hi_in), ldh, x_lo, ldl, lo_bits, gamma, beta, mod, ldmod, M, d,
                             rows_per_sample, eps, stream, x_hi_out);
}

extern "C" int swiftk_modnorm_residual_pair_slabs(const float* y_slabs, int64_t ldy, int64_t slab_stride, void* x_hi, int64_t ldh,
                                                  void* x_lo, int64_t ldl, int lo_bits, const float* gamma, const float* beta,
                                                  const float* mod, int64_t ldmod, int64_t M, int d, int64_t rows_per_sample,
                                                  float eps, void* stream) {
    if (slab_stride <= 0 || slab_stride % 4) return SWIFTK_EINVAL;
    return modnorm_pair_impl(y_slabs, ldy, slab_stride, x_hi, ldh, x_lo, ldl, lo_bits, gamma, beta, mod, ldmod, M, d,
                             rows_per_sample, eps, stream);
}

extern "C" int swiftk_modnorm_residual_pair_slabs_bf16(const void* y_slabs, int64_t ldy, int64_t slab_stride, void* x_hi, int64_t ldh,
                                                       void* x_lo, int64_t ldl, int lo_bits, const float* gamma, const float* beta,
                                                       const float* mod, int64_t ldmod, int64_t M, int d, int64_t rows_per_sample,
                                                       float eps, void* stream) {
    if (slab_stride <= 0 || slab_stride % 8) return SWIFTK_EINVAL;
    return modnorm_pair_impl(y_slabs, ldy, slab_stride, x_hi, ldh, x_lo, ldl, lo_bits, gamma, beta, mod, ldmod, M, d,
                             rows_per_sample, eps, stream, nullptr, true);
}

extern "C" int swiftk_modnorm_residual_pair_halves_bf16(const void* y_slabs, int64_t slab_stride, const int64_t* tail, void* x_hi, int64_t ldh,
                                                        void* x_lo, const float* gamma, const float* beta, const float* mod, int64_t ldmod,
                                                        int64_t M, int d, int64_t rows_per_sample, float eps, void* stream) {
    if (!y_slabs || !x_hi || !x_lo || !gamma || !beta || !mod || M <= 0 || rows_per_sample <= 0 || slab_stride <= 0) return SWIFTK_EINVAL;
    const int64_t rows_from = tail ? tail[0] : 0;
    const int tail_from = tail ? (int)tail[1] : 0, gm = tail ? (int)tail[2] : 8;
    if ((d != 1056 && d != 1280) || M % MN_ROWS || rows_per_sample % MN_ROWS || rows_from < 0 || rows_from > M || rows_from % MN_ROWS || ldh < d ||
        slab_stride < M * d || tail_from < 0 || gm < 1 || (tail_from > 0 && d != 1056))
        return SWIFTK_ESHAPE;
    if (((uintptr_t)y_slabs & 15) || (slab_stride * 2) % 16 || ((uintptr_t)x_hi & 15) || (ldh * 2) % 16 || ((uintptr_t)x_lo & 7) ||
        ((uintptr_t)gamma & 15) || ((uintptr_t)beta & 15) || ((uintptr_t)mod & 15) || (ldmod % 4))
        return SWIFTK_EALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bf16_t* y0 = static_cast<const bf16_t*>(y_slabs);
    bf16_t* hi = static_cast<bf16_t*>(x_hi);
    // The rows below rows_from have one y: they go through the one-y kernel (M = rows_from), the others through the two-slab form, which
    // starts at chunk rows_from / 16.  (One launch of the two-slab form over all rows, its two-slab chunks dealt evenly among the others, was
    // the first version: that instantiation moves every row 22 % slower than the one-y kernel, second slab or not -- 155.6 against 127.7 us
    // at twelve units with no row taking a second slab, `tools/halves_norm_bench.py`.)
    if (rows_from > 0) {
        const int g1 = (int)(rows_from / MN_ROWS);
        if (d == 1056)
            hipLaunchKernelGGL((modnorm_pair_packed_kernel<132>), dim3(g1), dim3(256), 0, st, y0, hi, hi, ldh, static_cast<uint8_t*>(x_lo), gamma, beta, mod,
                               ldmod, rows_from, rows_per_sample, eps, g_modnorm_nt);
        else
            hipLaunchKernelGGL((modnorm_pair_packed_kernel<160>), dim3(g1), dim3(256), 0, st, y0, hi, hi, ldh, static_cast<uint8_t*>(x_lo), gamma, beta, mod,
                               ldmod, rows_from, rows_per_sample, eps, g_modnorm_nt);
    }
    const int cgrid = (int)((M - rows_from) / MN_ROWS);
    const uint32_t chunk0 = (uint32_t)(rows_from / MN_ROWS);
    if (cgrid > 0) {
        if (d == 1056)
            hipLaunchKernelGGL((modnorm_pair_packed_kernel<132, true>), dim3(cgrid), dim3(256), 0, st, y0, hi, hi, ldh, static_cast<uint8_t*>(x_lo), gamma,
                               beta, mod, ldmod, M, rows_per_sample, eps, g_modnorm_nt, y0 + slab_stride, rows_from, tail_from, gm, chunk0);
        else
            hipLaunchKernelGGL((modnorm_pair_packed_kernel<160, true>), dim3(cgrid), dim3(256), 0, st, y0, hi, hi, ldh, static_cast<uint8_t*>(x_lo), gamma,
                               beta, mod, ldmod, M, rows_per_sample, eps, g_modnorm_nt, y0 + slab_stride, rows_from, tail_from, gm, chunk0);
    }
    SWIFTK_CHECK_LAUNCH();
    return 0;
}

extern "C" int swiftk_split_pair(const float* src, int64_t lds, void* hi, int64_t ldh, void* lo, int64_t ldl, int lo_bits,
                                 int64_t rows, int64_t cols, void* stream) {
    if (!src || !hi || !lo || rows <= 0 || cols <= 0 || (lo_bits != 16 && lo_bits != 8)) return SWIFTK_EINVAL;
    if (cols % 4 || ldh % 4 || ldl % 4 || lds % 4 || ldh < cols || ldl < cols || lds < cols) return SWIFTK_ESHAPE;
    if (((uintptr_t)src & 15) || ((uintptr_t)hi & 7) || ((uintptr_t)lo & 7)) return SWIFTK_EALIGN;
    hipLaunchKernelGGL(split_pair_kernel, dim3(grid_for(rows * (ldh >> 2))), dim3(256), 0, static_cast<hipStream_t>(stream), src,
                       lds, static_cast<bf16_t*>(hi), ldh, lo, ldl, rows, cols, lo_bits == 8 ? 1 : 0);
    SWIFTK_CHECK_LAUNCH();
    return 0;
}

extern "C" int swiftk_patchify_scaled(const float* src0, int c0, float s0, const float* s0_per_sample, const float* src1, int c1,
                                      float s1, const float* src2, int c2, float s2, void* A, int64_t lda, int B, int H, int W,
                                      int p1, int p2, int dtype, void* stream) {
    if (!A || !src0 || c0 <= 0 || c1 < 0 || c2 < 0 || B <= 0 || p1 <= 0 || p2 <= 0) return SWIFTK_EINVAL;
    if ((c1 > 0 && !src1) || (c2 > 0 && !src2)) return SWIFTK_EINVAL;
    if (H % p1 || W % p2) return SWIFTK_ESHAPE;
    PatchArgs a;
    a.src[0] = src0; a.src[1] = src1 ? src1 : src0; a.src[2] = src2 ? src2 : src0;
    a.cn[0] = c0; a.cn[1] = c1; a.cn[2] = c2;
    a.c0[0] = 0; a.c0[1] = c0; a.c0[2] = c0 + c1;
    if (c1 == 0) a.c0[1] = 1 << 30;
    if (c2 == 0) a.c0[2] = 1 << 30;
    a.sc[0] = s0; a.sc[1] = s1; a.sc[2] = s2;
    a.sc0 = s0_per_sample;
    a.B = B; a.H = H; a.W = W; a.p1 = p1; a.p2 = p2; a.C = c0 + c1 + c2; a.gh = H / p1; a.gw = W / p2;
    a.lda = lda;
    if (lda < (int64_t)p1 * p2 * a.C) return SWIFTK_ESHAPE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // tiled form where its alignment assumptions hold (16-token runs, float4 source segments, 16-B output chunks)
    const int rs = 16 * p2 + 4;
    const size_t tile_bytes = (size_t)a.C * p1 * rs * sizeof(float);
    bool aligned = !(a.gw & 15) && !((16 * p2) & 3) && !(W & 3) && !(lda & 7) && !((uintptr_t)A & 15) && tile_bytes <= 64 * 1024;
    for (int k = 0; k < 3; ++k) aligned = aligned && !((uintptr_t)a.src[k] & 15);
    if (aligned && (dtype == SWIFTK_BF16 || dtype == SWIFTK_F32)) {
        const dim3 grid(a.gw / 16, a.gh, B);
        if (dtype == SWIFTK_BF16)
            hipLaunchKernelGGL(patchify_tiled_kernel<bf16_t>, grid, dim3(256), tile_bytes, st, a, static_cast<bf16_t*>(A), rs);
        else
            hipLaunchKernelGGL(patchify_tiled_kernel<float>, grid, dim3(256), tile_bytes, st, a, static_cast<float*>(A), rs);
        SWIFTK_CHECK_LAUNCH();
        return 0;
    }
    const int grid = grid_for((int64_t)B * a.gh * a.gw * lda);
    if (dtype == SWIFTK_BF16)
        hipLaunchKernelGGL(patchify_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, a, static_cast<bf16_t*>(A));
    else if (dtype == SWIFTK_F32)
        hipLaunchKernelGGL(patchify_kernel<float>, dim3(grid), dim3(256), 0, st, a, static_cast<float*>(A));
    else
        return SWIFTK_EINVAL;
    SWIFTK_CHECK_LAUNCH();
    return 0;
}

extern "C" int swiftk_patchify(const float* src0, int c0, float s0, const float* src1, int c1, float s1, const float* src2,
                               int c2, float s2, void* A, int64_t lda, int B, int H, int W, int p1, int p2, int dtype,
                               void* stream) {
    return swiftk_patchify_scaled(src0, c0, s0, nullptr, src1, c1, s1, src2, c2, s2, A, lda, B, H, W, p1, p2, dtype, stream);
}

extern "C" int swiftk_unpatchify_affine(const float* tok, int64_t ldt, const float* xt, const float* alpha,
                                        const float* beta, float* out, int B, int C, int H, int W, int p1, int p2,
                                        void* stream) {
    if (!tok || !out || B <= 0 || C <= 0 || p1 <= 0 || p2 <= 0) return SWIFTK_EINVAL;
    if (H % p1 || W % p2 || ldt < (int64_t)C * p1 * p2) return SWIFTK_ESHAPE;
    if (p1 == 2 && p2 == 2 && W % 4 == 0 && ldt % 2 == 0 && !((uintptr_t)tok & 7) && !((uintptr_t)out & 15) && !((uintptr_t)xt & 15))
        hipLaunchKernelGGL(unpatchify4_kernel, dim3(grid_for((int64_t)B * C * H * (W / 4), 256, 1 << 20)), dim3(256), 0,
                           static_cast<hipStream_t>(stream), tok, ldt, xt, alpha, beta, out, B, C, H, W);
    else
        hipLaunchKernelGGL(unpatchify_kernel, dim3(grid_for((int64_t)B * C * H * W)), dim3(256), 0,
                           static_cast<hipStream_t>(stream), tok, ldt, xt, alpha, beta, out, B, C, H, W, p1, p2);
    SWIFTK_CHECK_LAUNCH();
    return 0;
}

extern "C" int swiftk_timestep_embed(const float* t, const float* aux, const float* freqs, const float* aux_w,
                                     const float* aux_b, float* emb, int B, int d, int aux_dim, float timestep_weight,
                                     void* stream) {
    if (!t || !freqs || !emb || B <= 0 || d <= 0) return SWIFTK_EINVAL;
    if (aux && aux_w && (!aux_b || aux_dim <= 0)) return SWIFTK_EINVAL;
    hipLaunchKernelGGL(temb_kernel, dim3((B * d + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), t, aux, freqs,
                       aux_w, aux_b, emb, B, d, aux_dim, timestep_weight);
    SWIFTK_CHECK_LAUNCH();
    return 0;
}

extern "C" int swiftk_linear_small(const float* x, int64_t ldx, const float* W, int64_t ldw, const float* bias, float* out,
                                   int64_t ldo, int B, int N, int K, int act, void* stream) {
    if (!x || !W || !out || B <= 0 || N <= 0 || K <= 0) return SWIFTK_EINVAL;
    if (((uintptr_t)x & 15) || ((uintptr_t)W & 15) || (ldx % 4) || (ldw % 4)) return SWIFTK_EALIGN;
    if (K % 4 == 0 && (size_t)8 * K * sizeof(float) <= 60 * 1024 && N >= 4096) {  // wide outputs: x staged in LDS
        const int grid = (N + 3) / 4 < 2048 ? (N + 3) / 4 : 2048;
        hipLaunchKernelGGL(linear_small_lds_kernel<8>, dim3(grid), dim3(256), (size_t)8 * K * sizeof(float),
                           static_cast<hipStream_t>(stream), x, ldx, W, ldw, bias, out, ldo, B, N, K, act);
        SWIFTK_CHECK_LAUNCH();
        return 0;
    }
    hipLaunchKernelGGL(linear_small_kernel<8>, dim3((N + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream), x, ldx, W,
                       ldw, bias, out, ldo, B, N, K, act);
    SWIFTK_CHECK_LAUNCH();
    return 0;
}

extern "C" int swiftk_rollout_update(float* xstd, const float* y, float* phys, const float* mx, const float* sx,
                                     const float* st, int B, int C, int64_t hw, void* stream) {
    if (!xstd || !y || !mx || !sx || B <= 0 || C <= 0 || hw <= 0) return SWIFTK_EINVAL;  // (st == NULL: non-residual form)
    if (hw % 4) return SWIFTK_ESHAPE;
    if (((uintptr_t)xstd & 15) || ((uintptr_t)y & 15) || (phys && ((uintptr_t)phys & 15))) return SWIFTK_EALIGN;
    const int64_t total4 = (int64_t)B * C * hw / 4;
    hipLaunchKernelGGL(rollout_update_kernel, dim3(grid_for(total4)), dim3(256), 0, static_cast<hipStream_t>(stream), xstd, y,
                       phys, mx, sx, st, C, hw / 4, total4);
    SWIFTK_CHECK_LAUNCH();
    return 0;
}

extern "C" int swiftk_cast_pad(const float* src, int64_t lds, void* dst, int64_t ldd, int64_t rows, int64_t cols,
                               int dtype, void* stream) {
    if (!src || !dst || rows <= 0 || cols <= 0 || ldd < cols || lds < cols) return SWIFTK_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int grid = grid_for(rows * ldd);
    if (dtype == SWIFTK_BF16)
        hipLaunchKernelGGL(cast_pad_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, src, lds, static_cast<bf16_t*>(dst), ldd,
                           rows, cols);
    else if (dtype == SWIFTK_F32)
        hipLaunchKernelGGL(cast_pad_kernel<float>, dim3(grid), dim3(256), 0, st, src, lds, static_cast<float*>(dst), ldd, rows,
                           cols);
    else
        return SWIFTK_EINVAL;
    SWIFTK_CHECK_LAUNCH();
    return 0;
}

// A trainable weight's two bf16 GEMM operands in one pass over the fp32 master copy: out[r'][c] = W[r][c] (row padding zeroed up to
// ldo) and out_t[c][r'] = the same value (padding zeroed up to ldt), r' = r or, for w1, the (gate, up)-interleaved row 2 (r % inter)
// + r / inter.  64 x 64 tiles through LDS; both stores walk consecutive addresses.
__global__ __launch_bounds__(256) void cast_pad_t_kernel(const float* __restrict__ W, int64_t ldw, int rows, int cols,
                                                         bf16_t* __restrict__ out, int64_t ldo, bf16_t* __restrict__ out_t, int64_t ldt,
                                                         int inter) {
    __shared__ float tile[64][65];
    const int c0 = blockIdx.x * 64, r0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int rp = r0 + ty + 4 * k, c = c0 + tx;
        float v = 0.f;
        if (rp < rows && c < cols) {
            const int r = inter ? (rp & 1) * inter + (rp >> 1) : rp;
            v = W[(int64_t)r * ldw + c];
        }
        tile[ty + 4 * k][tx] = v;
        if (rp < rows && c < ldo) out[(int64_t)rp * ldo + c] = f2bf(v);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int c = c0 + ty + 4 * k, rp = r0 + tx;
        if (c < cols && rp < ldt) out_t[(int64_t)c * ldt + rp] = f2bf(tile[tx][ty + 4 * k]);
    }
}

extern "C" int swiftk_cast_pad_t(const float* W, int64_t ldw, int64_t rows, int64_t cols, void* out, int64_t ldo, void* out_t,
                                 int64_t ldt, int64_t interleave, void* stream) {
    if (!W || !out || !out_t || rows <= 0 || cols <= 0 || ldw < cols || ldo < cols || ldt < rows) return SWIFTK_EINVAL;
    if (rows > (1 << 30) || cols > (1 << 30) || ldo > (1 << 30) || ldt > (1 << 30)) return SWIFTK_ESHAPE;
    if (interleave < 0 || (interleave > 0 && rows != 2 * interleave)) return SWIFTK_ESHAPE;
    const int64_t rmax = rows > ldt ? rows : ldt, cmax = cols > ldo ? cols : ldo;
    const dim3 grid((unsigned)((cmax + 63) / 64), (unsigned)((rmax + 63) / 64));
    if (grid.y > 65535) return SWIFTK_ESHAPE;
    hipLaunchKernelGGL(cast_pad_t_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), W, ldw, (int)rows, (int)cols,
                       static_cast<bf16_t*>(out), ldo, static_cast<bf16_t*>(out_t), ldt, (int)interleave);
    SWIFTK_CHECK_LAUNCH();
    return 0;
}

// swiftk_cast_pad_t without the interleave, with the head-lane map on one axis (zero-padded head lanes): along that axis output index
// b * hdp + j reads parameter index b * hd + j for j < hd and is zero for hd <= j < hdp.  Tiles are 64 x 64 of the OUTPUT (lane-shaped)
// index space; both stores walk consecutive addresses and write every element of both buffers once, the zero lanes and the row paddings
// included.  rl / cl: the lane-shaped extents.
__device__ __forceinline__ int lane_src(int p, int hd, int hdp) {  // parameter index of lane-shaped index p, -1 on a pad lane
    const int b = p / hdp, j = p - b * hdp;
    return j < hd ? b * hd + j : -1;
}

__global__ __launch_bounds__(256) void cast_pad_t_lanes_kernel(const float* __restrict__ W, int64_t ldw, int rl, int cl,
                                                               bf16_t* __restrict__ out, int64_t ldo, bf16_t* __restrict__ out_t,
                                                               int64_t ldt, int axis, int hd, int hdp) {
    __shared__ float tile[64][65];
    const int c0 = blockIdx.x * 64, r0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int cp = c0 + tx;
    const int c = cp >= cl ? -1 : (axis == 1 ? lane_src(cp, hd, hdp) : cp);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int rp = r0 + ty + 4 * k;
        float v = 0.f;
        if (rp < rl && c >= 0) {
            const int r = axis == 0 ? lane_src(rp, hd, hdp) : rp;
            if (r >= 0) v = W[(int64_t)r * ldw + c];
        }
        tile[ty + 4 * k][tx] = v;
        if (rp < rl && cp < ldo) out[(int64_t)rp * ldo + cp] = f2bf(v);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int ct = c0 + ty + 4 * k, rp = r0 + tx;
        if (ct < cl && rp < ldt) out_t[(int64_t)ct * ldt + rp] = f2bf(tile[tx][ty + 4 * k]);
    }
}

extern "C" int swiftk_cast_pad_t_lanes(const float* W, int64_t ldw, int64_t rows, int64_t cols, void* out, int64_t ldo, void* out_t,
                                       int64_t ldt, int axis, int64_t blocks, int64_t hd, int64_t hdp, void* stream) {
    if (!W || !out || !out_t || rows <= 0 || cols <= 0 || blocks <= 0 || hd <= 0 || hdp < hd || ldw < cols) return SWIFTK_EINVAL;
    if (axis != 0 && axis != 1) return SWIFTK_EINVAL;
    if (rows > (1 << 30) || cols > (1 << 30) || ldo > (1 << 30) || ldt > (1 << 30) || blocks > (1 << 30) || hdp > (1 << 30) ||
        blocks * hdp > (1 << 30))
        return SWIFTK_ESHAPE;
    if ((axis == 0 ? rows : cols) != blocks * hd) return SWIFTK_ESHAPE;
    const int64_t rl = axis == 0 ? blocks * hdp : rows, cl = axis == 1 ? blocks * hdp : cols;  // lane-shaped extents
    if (ldo < cl || ldt < rl) return SWIFTK_EINVAL;
    const int64_t rmax = rl > ldt ? rl : ldt, cmax = cl > ldo ? cl : ldo;
    const dim3 grid((unsigned)((cmax + 63) / 64), (unsigned)((rmax + 63) / 64));
    if (grid.y > 65535) return SWIFTK_ESHAPE;
    hipLaunchKernelGGL(cast_pad_t_lanes_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), W, ldw, (int)rl, (int)cl,
                       static_cast<bf16_t*>(out), ldo, static_cast<bf16_t*>(out_t), ldt, axis, (int)hd, (int)hdp);
    SWIFTK_CHECK_LAUNCH();
    return 0;
}

// Adjoint of the lane map on a weight gradient: G[r][c] += g[map(r)][c] (axis 0) or g[r][map(c)] (axis 1), map(b * hd + j) = b * hdp + j.
// One thread per V consecutive columns of G (V = 4, 2 or 1: the widest that keeps a vector inside one head's valid lanes and aligned).
template <int V>
__global__ __launch_bounds__(256) void lanes_grad_add_kernel(float* __restrict__ G, int64_t ldg, const float* __restrict__ g, int64_t ldl,
                                                             int cols, int64_t total, int axis, int hd, int hdp) {
    const int cv = cols / V;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / cv), c = (int)(i - (int64_t)r * cv) * V;
        int rs = r, cs = c;
        if (axis == 0) rs = r / hd * hdp + r % hd;
        else cs = c / hd * hdp + c % hd;
        float* pg = G + (int64_t)r * ldg + c;
        const float* ps = g + (int64_t)rs * ldl + cs;
        if constexpr (V == 4) {
            float4 a = *reinterpret_cast<float4*>(pg);
            const float4 b = *reinterpret_cast<const float4*>(ps);
            a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
            *reinterpret_cast<float4*>(pg) = a;
        } else if constexpr (V == 2) {
            float2 a = *reinterpret_cast<float2*>(pg);
            const float2 b = *reinterpret_cast<const float2*>(ps);
            a.x += b.x; a.y += b.y;
            *reinterpret_cast<float2*>(pg) = a;
        } else {
            *pg += *ps;
        }
    }
}

extern "C" int swiftk_lanes_grad_add(float* G, int64_t ldg, const float* g, int64_t ldl, int64_t rows, int64_t cols, int axis,
                                     int64_t blocks, int64_t hd, int64_t hdp, void* stream) {
    if (!G || !g || rows <= 0 || cols <= 0 || blocks <= 0 || hd <= 0 || hdp < hd || ldg < cols) return SWIFTK_EINVAL;
    if (axis != 0 && axis != 1) return SWIFTK_EINVAL;
    if (rows > (1 << 30) || cols > (1 << 30) || blocks > (1 << 30) || hdp > (1 << 30) || blocks * hdp > (1 << 30)) return SWIFTK_ESHAPE;
    if ((axis == 0 ? rows : cols) != blocks * hd) return SWIFTK_ESHAPE;
    if (ldl < (axis == 1 ? blocks * hdp : cols)) return SWIFTK_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const auto fits = [&](int64_t v) {  // vectors of v floats: whole ones per row, never across a lane boundary, aligned on both sides
        return cols % v == 0 && ldg % v == 0 && ldl % v == 0 && (axis == 0 || (hd % v == 0 && hdp % v == 0)) &&
               !((uintptr_t)G & (4 * v - 1)) && !((uintptr_t)g & (4 * v - 1));
    };
    const int V = fits(4) ? 4 : (fits(2) ? 2 : 1);
    const int64_t total = rows * (cols / V);
    const dim3 grid(grid_for(total));
    if (V == 4)
        hipLaunchKernelGGL(lanes_grad_add_kernel<4>, grid, dim3(256), 0, st, G, ldg, g, ldl, (int)cols, total, axis, (int)hd, (int)hdp);
    else if (V == 2)
        hipLaunchKernelGGL(lanes_grad_add_kernel<2>, grid, dim3(256), 0, st, G, ldg, g, ldl, (int)cols, total, axis, (int)hd, (int)hdp);
    else
        hipLaunchKernelGGL(lanes_grad_add_kernel<1>, grid, dim3(256), 0, st, G, ldg, g, ldl, (int)cols, total, axis, (int)hd, (int)hdp);
    SWIFTK_CHECK_LAUNCH();
    return 0;
}

extern "C" int swiftk_split3(const float* src, int64_t lds, void* dst, int64_t ldd, int64_t rows, int64_t cols, int order,
                             void* stream) {
    if (!src || !dst || rows <= 0 || cols <= 0 || lds < cols || ldd < 3 * cols || (order != 0 && order != 1)) return SWIFTK_EINVAL;
    if (cols % 4 || ldd % 4 || lds % 4) return SWIFTK_ESHAPE;
    if (((uintptr_t)src & 15) || ((uintptr_t)dst & 7)) return SWIFTK_EALIGN;
    hipLaunchKernelGGL(split3_kernel, dim3(grid_for(rows * ((ldd - 2 * cols) >> 2))), dim3(256), 0, static_cast<hipStream_t>(stream),
                       src, lds, static_cast<bf16_t*>(dst), ldd, rows, cols, order);
    SWIFTK_CHECK_LAUNCH();
    return 0;
}

extern "C" int swiftk_unit_noise(float* out, const int64_t* seeds, const int64_t* step, int64_t step_add, int B,
                                 int64_t n_per_unit, int mode, void* stream) {
    if (!out || !seeds || B <= 0 || n_per_unit <= 0 || (mode != 0 && mode != 1)) return SWIFTK_EINVAL;
    if (n_per_unit % 4 || B > 65535) return SWIFTK_ESHAPE;
    if ((uintptr_t)out & 15) return SWIFTK_EALIGN;
    const int64_t n4 = n_per_unit / 4;
    hipLaunchKernelGGL(unit_noise_kernel, dim3(grid_for(n4, 256, 1024), B), dim3(256), 0, static_cast<hipStream_t>(stream), out,
                       seeds, step, step_add, n4, mode);
    SWIFTK_CHECK_LAUNCH();
    return 0;
}

extern "C" int swiftk_counter_add(int64_t* counter, int64_t value, void* stream) {
    if (!counter) return SWIFTK_EINVAL;
    hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), counter, value);
    SWIFTK_CHECK_LAUNCH();
    return 0;
}

int g_zero_memset = 0;  // tuning key 25 (diagnosis only), bit mask: 1 = the library's internal clears (swiftk_modnorm_bwd's column-sum
                        // workspace, swiftk_scm_target's scratch), 2 = the exported swiftk_zero_f32 -- through hipMemsetAsync, the round-4/5 form

int swiftk_zero_f32_impl(float* p, int64_t n, void* stream, int who) {
    if (!p || n < 0) return SWIFTK_EINVAL;
    if (n == 0) return 0;
    if (((uintptr_t)p & 3)) return SWIFTK_EALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (g_zero_memset & who) return (int)hipMemsetAsync(p, 0, sizeof(float) * (size_t)n, st);
    return swiftk_zero_f32_launch(p, n, st);
}

extern "C" int swiftk_zero_f32(float* p, int64_t n, void* stream) { return swiftk_zero_f32_impl(p, n, stream, 2); }

// Diagnosis of the round-5 overflow (tuning key 25, bit 4): a check kernel right behind a clear counts what the clear left
// non-zero -- per dword index mod 4, with the largest magnitude and a few (index, bits) samples -- into a small device record
// that swiftk_zero_check_report copies out.  The record is allocated when the bit is set (never inside a stream capture).
namespace {
struct ZeroCheck {
    unsigned long long calls, bad[4];
    unsigned int worst[4];
    unsigned int n_samples, sample_idx[8], sample_bits[8];
};
ZeroCheck* g_zero_check = nullptr;

__global__ __launch_bounds__(256) void zero_check_kernel(const unsigned int* __restrict__ p, int64_t n, ZeroCheck* rec) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&rec->calls, 1ull);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const unsigned int v = p[i];
        if (v != 0u) {
            atomicAdd(&rec->bad[i & 3], 1ull);
            atomicMax(&rec->worst[i & 3], v & 0x7fffffffu);
            const unsigned int k = atomicAdd(&rec->n_samples, 1u);
            if (k < 8) {
                rec->sample_idx[k] = (unsigned int)i;
                rec->sample_bits[k] = v;
            }
        }
    }
}
}  // namespace

int swiftk_zero_check_enable() {
    if (g_zero_check) return 0;
    if (hipMalloc(reinterpret_cast<void**>(&g_zero_check), sizeof(ZeroCheck)) != hipSuccess) return SWIFTK_EINVAL;
    return hipMemset(g_zero_check, 0, sizeof(ZeroCheck)) == hipSuccess ? 0 : SWIFTK_EINVAL;
}

int swiftk_zero_check_launch(const float* p, int64_t n, void* stream) {
    if (!g_zero_check) return 0;
    const int64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(zero_check_kernel, dim3((unsigned)(blocks < 256 ? (blocks < 1 ? 1 : blocks) : 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), reinterpret_cast<const unsigned int*>(p), n, g_zero_check);
    return (int)hipGetLastError();
}

/* out[0] = checks run, out[1..4] = non-zero dwords found by index mod 4, out[5..8] = largest |bits| by index mod 4,
 * out[9] = samples, out[10..17] = sample indices, out[18..25] = sample bits (device synchronisation; diagnosis only) */
extern "C" int swiftk_zero_check_report(unsigned long long* out26) {
    if (!out26) return SWIFTK_EINVAL;
    for (int i = 0; i < 26; ++i) out26[i] = 0;
    if (!g_zero_check) return 0;
    ZeroCheck h;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(&h, g_zero_check, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return SWIFTK_EINVAL;
    out26[0] = h.calls;
    for (int i = 0; i < 4; ++i) { out26[1 + i] = h.bad[i]; out26[5 + i] = h.worst[i]; }
    out26[9] = h.n_samples;
    for (int i = 0; i < 8; ++i) { out26[10 + i] = h.sample_idx[i]; out26[18 + i] = h.sample_bits[i]; }
    return 0;
}

extern "C" int swiftk_axpby(float* out, float a, const float* x, float b, const float* y, int64_t n, void* stream) {
    if (!out || !x || !y || n <= 0) return SWIFTK_EINVAL;
    if (((uintptr_t)out & 15) || ((uintptr_t)x & 15) || ((uintptr_t)y & 15)) return SWIFTK_EALIGN;
    hipLaunchKernelGGL(axpby_kernel, dim3(grid_for(n / 4 + 1)), dim3(256), 0, static_cast<hipStream_t>(stream), out, a, x, b, y,
                       n / 4, n);
    SWIFTK_CHECK_LAUNCH();
    return 0;
}

extern "C" int swiftk_unit_checksum(const float* x, double* out, double* scratch, int B, int64_t n, void* stream) {
    if (!x || !out || !scratch || B <= 0 || n <= 0) return SWIFTK_EINVAL;
    if (n % 4) return SWIFTK_ESHAPE;
    if ((uintptr_t)x & 15) return SWIFTK_EALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(checksum_part_kernel, dim3(CK_PARTS, B), dim3(256), 0, st, x, scratch, n);
    hipLaunchKernelGGL(checksum_final_kernel, dim3((B + 63) / 64), dim3(64), 0, st, scratch, out, B);
    SWIFTK_CHECK_LAUNCH();
    return 0;
}

extern "C" int swiftk_version(void) { return 3; }
