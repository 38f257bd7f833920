// Persistent, LDS-DMA-streamed shifted-window attention for gfx950 (bf16, head_dim 80 / 88 / 96, pre-normalised q/k;
// the text below describes the Swift-B geometry, head_dim 88).
//
// The to_qkv GEMM epilogue (SWIFTK_EPI_QKNORM) has already L2-normalised q and k and applied the logit scale,
// so this kernel is pure data movement + MFMA + softmax.  A (sample, window, head) item is 3 x 45 KB in and
// 45 KB out for 23 MFLOP x 2: HBM-bound, so the design goal is an HBM stream that never
// stops while the matrix pipe and the VALU work underneath it:
//   * a fixed grid of workgroups walks contiguous runs of items (heads fastest: the twelve 528-B [q|k|v] slices of
//     a token are neighbours in memory and are consumed back to back by the same CU);
//   * every input byte travels HBM -> LDS by global_load_lds (no VGPR round trip, no VALU, 16 B per lane with
//     whole 176-B row segments per instruction).  K and V stream through a ring of four 64-key stages three
//     stages ahead of the compute; the Q tile of the NEXT item is requested a whole item ahead into a buffer that
//     the waves drain into registers at the start of each item;
//   * softmax is streamed over the four key chunks.  |logit| <= |q||k| = exp(min(scale, ln 100)) because q and k
//     arrive normalised; when that bound is <= 48 no maximum is needed at all (offset 0 is as exact as any other
//     in floating point, and e^48 * 256 * |v| is far inside the fp32 / bf16 range).  Heads with a larger bound
//     use the running-maximum (online) form: each lane owns one query column, so the rescale is a per-lane scalar;
//   * the row sum l rides on the matrix pipe (ones fed to the unused V^T rows d = 88..95), so rescaling O
//     rescales l with it;
//   * the output tile of item i leaves during item i+1 through wave-private LDS slabs, as whole 176-B row
//     segments per dwordx4 store;
//   * waits are counted: VMEM retires in issue order, so `s_waitcnt vmcnt(N)` with N = the operations issued
//     after the stage that is needed leaves the younger prefetches in flight across the barrier.
// Rows are 88 bf16 = 176 B, unpadded: 16 consecutive rows hit 16 distinct 16-B bank slots (176/16 = 11 is odd), so
// the ds_read_b128 fragment reads are conflict-free; the k-step that covers d = 80..95 reads 16 B into the next row
// for d >= 88 and meets a zero Q fragment (all LDS is zero-filled once, so those bits are finite).
// MFMA orientation and the accumulator-as-operand trick are those of attention.hip.
#include "common.h"

int g_attn_dbg = 0;
int g_attn_pp = 1;  // tuning key 21 (qkv_attn.hip): ping-pong k-loop of the fused to_qkv + attention kernel
int g_attn_sl = 3;  // tuning key 30 (qkv_attn.hip): bit 0 straight-line hand-off, bit 1 straight-line output stage + item decode

namespace {

constexpr int NT = 512;
constexpr int CH = 64;                  // keys per ring stage
constexpr int NST = 4;                  // ring stages = chunks per item
constexpr int DB = 3;                   // 32-row blocks of O^T (head_dim <= 96)
constexpr float LOG2E = 1.4426950408889634f;

// Geometry by head_dim (80 / 88 / 96: the 468 M, Swift-B and 664 M variants; comments below quote the 88 numbers).
template <int HD>
struct Geo {
    static constexpr int CPR = HD / 8;             // 16-B chunks per row: 10 / 11 / 12
    static constexpr int ROW = HD * 2;             // 176 B
    static constexpr int TILE = 256 * ROW;         // 45056 B = 44 DMA pieces
    static constexpr int NPQ = TILE / 1024;        // pieces of a Q / K / V tile: 40 / 44 / 48
    static constexpr int CHB = CH * ROW;           // 11264 B = 11 pieces
    static constexpr int NPC = CHB / 1024;         // pieces of one K (or V) chunk: 10 / 11 / 12
    static constexpr int OROWS = HD > 88 ? 8 : 16;  // query rows per output round (head_dim 96: 8, or LDS would not fit)
    static constexpr int ORND = 32 / OROWS;         // rounds per item (a wave owns 32 queries)
    static constexpr int NOST = ORND * ((OROWS * CPR + 63) / 64);  // output store instructions per wave and item: 6 / 6 / 8
    static constexpr int OSLAB = OROWS * ROW;       // per-wave output staging slab (2816 B)
    static constexpr int OFF_K = TILE;             // Q tile | K ring | V ring | zero tail | output slabs
    static constexpr int OFF_V = OFF_K + NST * CHB;
    static constexpr int OFF_O = OFF_V + NST * CHB + 64;
    static constexpr int LDS_TOTAL = OFF_O + 8 * OSLAB;
    static constexpr int KS = (HD + 15) / 16;      // 16-wide k-steps of S = K Q^T: 5 / 6 / 6
    static constexpr bool ONES = HD < 32 * DB;     // spare V^T rows carry ones -> the row sum rides on the matrix pipe
};

__device__ __forceinline__ int win_token(int wy, int wx, int j, int gh, int gw, int sh, int sw) {
    int gy = wy * 16 + (j >> 4) + sh;
    int gx = wx * 16 + (j & 15) + sw;
    gy = gy >= gh ? gy - gh : gy;
    gx = gx >= gw ? gx - gw : gx;
    return gy * gw + gx;
}

template <int N>
__device__ __forceinline__ void wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// DBG: ablation bits for timing experiments (1 no steady-state K/V DMA, 2 no S/softmax/PV, 4 no steady-state Q DMA,
// 8 no O stores)
template <int DBG, int HD>
__global__ __launch_bounds__(NT) void attn_pipe_kernel(AttnPipeArgs a, int nitems) {
    using G = Geo<HD>;
    constexpr int CPR = G::CPR, ROW = G::ROW, TILE = G::TILE, NPQ = G::NPQ, CHB = G::CHB, NPC = G::NPC, OSLAB = G::OSLAB;
    constexpr int OFF_K = G::OFF_K, OFF_V = G::OFF_V, OFF_O = G::OFF_O, LDS_TOTAL = G::LDS_TOTAL, KS = G::KS;
    constexpr int OROWS = G::OROWS, ORND = G::ORND, NOST = G::NOST;
    __shared__ __attribute__((aligned(16))) char smem[LDS_TOTAL];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nwx = a.gw / 16, nw = (a.gh / 16) * nwx;
    const int64_t ldq_b = a.ldq * 2;
    const int64_t ntok = (int64_t)a.gh * a.gw;

    // contiguous run of items for this workgroup (items of one window are adjacent: heads fastest)
    // Item order.  Items are numbered (sample, window, head), heads fastest.  The workgroups that share an XCD
    // (blockIdx & 7: they share its L2) take CONSECUTIVE items at the same time, each XCD walking its own contiguous
    // eighth of the list in rounds: the 176-B head slices of a token row are neighbours in memory, so partial cache
    // lines -- the output's above all, which would otherwise go back to HBM half-written and be merged there by
    // read-modify-write -- are completed in L2 by the neighbouring CUs while they are still resident.
    // (Measured at 8 samples: 157 us with one contiguous run per workgroup, 140 us in this order.)
    int first, last, istep;
    if ((gridDim.x & 7) == 0) {
        const int xcd = blockIdx.x & 7, nx = gridDim.x >> 3;
        first = (int)((int64_t)xcd * nitems / 8) + (blockIdx.x >> 3);
        last = (int)((int64_t)(xcd + 1) * nitems / 8);
        istep = nx;
    } else {
        first = (int)((int64_t)blockIdx.x * nitems / gridDim.x);
        last = (int)((int64_t)(blockIdx.x + 1) * nitems / gridDim.x);
        istep = 1;
    }
    if (first >= last) return;

    // zero all LDS once: the 16-B over-reads behind a row / a stage must see finite bits
    for (int o = tid * 16; o < LDS_TOTAL; o += NT * 16) *reinterpret_cast<uint4*>(smem + o) = make_uint4(0, 0, 0, 0);
    __syncthreads();
    const uint32_t lds0 = (uint32_t)(uintptr_t)LDS_PTR(smem);

    const int c32 = lane & 31, hh = lane >> 5;
    const int i16 = lane & 15;
    const int vbase = (4 * hh + (i16 >> 2)) * ROW + (16 * ((lane >> 4) & 1) + 4 * (i16 & 3)) * 2;

    // ---- DMA bookkeeping.  A piece is 1 KiB = 64 lanes x 16 B; piece p of a 256-row tile covers its 16-B chunks
    // 64p .. 64p+63 (chunk c -> row c/11, chunk c%11 of the row), i.e. 5.8 whole 176-B row segments.
    //   Q tile: 44 pieces, wave wv issues slots wv + 8i, i = 0..5; slots 44..47 repeat pieces 0..3 (same bytes to the
    //           same place) so that every wave issues exactly 6 -- the counted waits below need uniform counts;
    //   K/V chunk c: 11 + 11 pieces (tile pieces 11c .. 11c+10 of K, then of V), wave wv issues slots wv + 8s,
    //           s = 0..2; slots 22, 23 repeat slots 0, 1.
    // Per-lane source offsets depend on the window only; they are recomputed when the window changes.
    uint32_t qoff[6], coff[NST][3];
    int cur_w = -1;
    int tb_w = 0;  // window of the item the DMA helpers are fetching (tiled storage addresses tiles by window)
    auto piece_off = [&](int wy, int wx, int p) {
        const int c = p * 64 + lane;
        const int row = c / CPR;  // (a constant divisor: multiply-shift)
        const int cc = c - row * CPR;
        if (a.tiled) return (uint32_t)(p * 1024 + lane * 16);  // window-tiled storage: a tile is one contiguous block
        return (uint32_t)(win_token(wy, wx, row, a.gh, a.gw, a.sh, a.sw) * ldq_b) + 16u * cc;
    };
    int cslot_part[3], cslot_j[3];  // wave-uniform: which tensor (0 K, 1 V) and which piece of the chunk a slot is
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        int q = wv + 8 * s;
        q = q >= 2 * NPC ? q - 2 * NPC : q;
        cslot_part[s] = q >= NPC;
        cslot_j[s] = q - NPC * cslot_part[s];
    }
    auto set_window = [&](int w) {
        const int wy = w / nwx, wx = w - wy * nwx;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            int p = wv + 8 * i;
            p = p >= NPQ ? p - NPQ : p;
            qoff[i] = piece_off(wy, wx, p);
        }
#pragma unroll
        for (int c = 0; c < NST; ++c)
#pragma unroll
            for (int s = 0; s < 3; ++s) coff[c][s] = piece_off(wy, wx, NPC * c + cslot_j[s]);
        cur_w = w;
    };
    auto decode = [&](int item, int& b, int& w, int& h) {
        h = item % a.heads;
        const int r = item / a.heads;
        w = r % nw;
        b = r / nw;
    };
    // tile base of (b, h): part 0 = q, 1 = k, 2 = v
    auto tile_base = [&](int b, int h, int part) {
        if (a.tiled)
            return static_cast<const char*>(a.qkv) + (((int64_t)(b * nw + tb_w) * a.heads + h) * 3 + part) * TILE;
        return static_cast<const char*>(a.qkv) + (int64_t)b * ntok * ldq_b + (int64_t)(h * 3 + part) * ROW;
    };
    auto pin = [&](const char* base) {  // keep a provably wave-uniform pointer in SGPRs for the asm operand
        const uint64_t u = (uint64_t)base;
        return (const char*)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(u >> 32)) << 32) |
                             (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)u));
    };
    auto dma_q = [&](int b, int h) {
        const char* base = pin(tile_base(b, h, 0));
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            int p = wv + 8 * i;
            p = p >= NPQ ? p - NPQ : p;
            dma_piece(lds0 + p * 1024, base, qoff[i]);
        }
    };
    auto dma_chunk = [&](int b, int h, int c) {  // chunk c of the item -> ring stage c
        const char* kb_ = pin(tile_base(b, h, 1));
        const char* vb_ = pin(tile_base(b, h, 2));
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const uint32_t dst = lds0 + (cslot_part[s] ? OFF_V : OFF_K) + c * CHB + cslot_j[s] * 1024;
            dma_piece(__builtin_amdgcn_readfirstlane(dst), cslot_part[s] ? vb_ : kb_, coff[c][s]);
        }
    };

    f32x16 o[DB];  // output of the current item; stored one step into the next item
    float rl_prev = 0.f;
    int pb = 0, pw = 0, ph = 0;
    bool have_prev = false;
    // The output tile leaves through a wave-private LDS slab (16 rows x 176 B, two rounds per item): written as the
    // 8-B pieces the MFMA layout yields (row stride 176 B = 44 banks: 16 rows land on 16 distinct bank groups), read
    // back as whole 16-B chunks of consecutive row bytes, so one dwordx4 store covers ~5.8 complete 176-B row
    // segments instead of 32 rows x 16 B.  Always exactly 6 store instructions per wave (counted waits).
    char* oslab = smem + OFF_O + wv * OSLAB;
    auto store_o = [&](int b, int w, int h, float rl) {
        const int wy = w / nwx, wx = w - wy * nwx;
        bf16_t* obase = static_cast<bf16_t*>(a.out) + (int64_t)b * ntok * a.ldo + h * HD;
#pragma unroll
        for (int rnd = 0; rnd < ORND; ++rnd) {
            if (c32 / OROWS == rnd) {
#pragma unroll
                for (int db = 0; db < DB; ++db)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int d = db * 32 + g * 8 + hh * 4;
                        if (d < HD)
                            *reinterpret_cast<uint2*>(oslab + (c32 & (OROWS - 1)) * ROW + d * 2) =
                                make_uint2(pack_bf16(o[db][4 * g] * rl, o[db][4 * g + 1] * rl),
                                           pack_bf16(o[db][4 * g + 2] * rl, o[db][4 * g + 3] * rl));
                    }
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int t = 0; t < (OROWS * CPR + 63) / 64; ++t) {
                const int c = lane + 64 * t;
                if (c < OROWS * CPR) {
                    const int row = c / CPR, cc = c - row * CPR;
                    const uint4 v = *reinterpret_cast<const uint4*>(oslab + row * ROW + cc * 16);
                    const int tok = win_token(wy, wx, wv * 32 + rnd * OROWS + row, a.gh, a.gw, a.sh, a.sw);
                    *reinterpret_cast<uint4*>(obase + (int64_t)tok * a.ldo + cc * 8) = v;
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    };

    // ---- prologue, in the order the steady state issues (chunk 0, Q, chunk 1, chunk 2 of the coming item)
    int b, w, h;
    decode(first, b, w, h);
    set_window(w);
    tb_w = w;
    dma_chunk(b, h, 0);
    dma_q(b, h);
    dma_chunk(b, h, 1);
    dma_chunk(b, h, 2);

    const uint4 ones = make_uint4(0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u);
    for (int item = first; item < last; item += istep) {
        // the item after this one; past the end of the run the "next item" is this one again: the re-loads put the
        // same bytes where they already are and keep every count below uniform
        int nb = b, nwn = w, nh = h;
        if (item + istep < last) decode(item + istep, nb, nwn, nh);
        const float bound = a.scale ? __expf(fminf(a.scale[h], 4.605170185988092f)) : INFINITY;
        const bool online = !(bound <= 48.f);
        float m_run = -INFINITY;  // running row maximum (online form only)
        float l_valu = 0.f;       // head_dim 96 only: no spare V^T rows, the row sum is added up on the VALU
        uint4 qf[KS];

#pragma unroll
        for (int c = 0; c < NST; ++c) {
            // ---- hand-over of stage c.  Younger VMEM operations that may stay in flight (per wave, issue order):
            //  c = 0: needs chunk 0 and Q of this item (Q was issued right after chunk 0): chunk 1, chunk 2       = 6
            //  c = 1: chunk 2, chunk 3 (step 0), O stores (step 0; none on the first item)                       = 12 / 6
            //  c = 2: chunk 3, O stores, next chunk 0 + next Q (step 1)                                          = 18 / 12
            //  c = 3: O stores, next chunk 0, next Q, next chunk 1 (step 2)                                      = 18 / 12
            if (DBG & 5) {
                wait_vm<0>();
            } else if (c == 0) {
                wait_vm<6>();
            } else if (c == 1) {
                if (have_prev && !(DBG & 8)) wait_vm<6 + NOST>(); else wait_vm<6>();
            } else {
                if (have_prev && !(DBG & 8)) wait_vm<12 + NOST>(); else wait_vm<12>();
            }
            __builtin_amdgcn_s_barrier();
            // every wave's pieces of stage c have landed, and every wave is done with stage c-1 (its fragment reads
            // were consumed by MFMAs before it arrived here) -> refill that stage with the chunk three ahead
            if (c == 0) {
                tb_w = w;
                if (!(DBG & 1)) dma_chunk(b, h, 3);
                // Q fragments of query row 32*wv + c32: chunk 2*ks + hh of the row (chunk 11 does not exist -> zeros)
                const char* qrow = smem + (wv * 32 + c32) * ROW;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    if (ks == KS - 1 && (CPR & 1)) {  // odd chunk count (head_dim 88): the last k-step has one real chunk
                        const uint4 t = *reinterpret_cast<const uint4*>(qrow + (2 * ks) * 16);
                        qf[ks] = hh ? make_uint4(0, 0, 0, 0) : t;
                    } else {
                        qf[ks] = *reinterpret_cast<const uint4*>(qrow + (2 * ks + hh) * 16);
                    }
                }
                if (have_prev) {
                    if (!(DBG & 8)) store_o(pb, pw, ph, rl_prev);
                }
                // only now may the accumulators be recycled for this item
#pragma unroll
                for (int db = 0; db < DB; ++db)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
            } else {
                if (c == 1 && nwn != cur_w && !a.tiled) set_window(nwn);
                tb_w = nwn;
                if (!(DBG & 1)) dma_chunk(nb, nh, c - 1);
                // every wave has its Q fragments in registers (they were consumed by step 0's MFMAs): the buffer
                // takes the next item's Q, a whole item ahead of its use
                if (c == 1 && !(DBG & 4)) dma_q(nb, nh);
            }
            if constexpr (DBG & 2) continue;

            // S^T[key][q] = K Q^T for the 64 keys of this stage, as two 32-key blocks
            const char* sK = smem + OFF_K + c * CHB;
            const char* sV = smem + OFF_V + c * CHB;
            f32x16 sc[2];
#pragma unroll
            for (int k2 = 0; k2 < 2; ++k2) {
#pragma unroll
                for (int r = 0; r < 16; ++r) sc[k2][r] = 0.f;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const uint4 kf = *reinterpret_cast<const uint4*>(sK + (k2 * 32 + c32) * ROW + ks * 32 + hh * 16);
                    sc[k2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, kf),
                                                                     __builtin_bit_cast(bf16x8, qf[ks]), sc[k2], 0, 0, 0);
                }
            }
            float mb = 0.f;
            if (online) {
                // running maximum of query column c32 (this lane's 32 values and lane^32's), rescale O and l with it
                float mx = m_run;
#pragma unroll
                for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
                    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sc[k2][r]);
                mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
                const float alpha = __builtin_amdgcn_exp2f((m_run - mx) * LOG2E);  // 0 on the first chunk (O is 0 too)
                m_run = mx;
                mb = mx * LOG2E;
#pragma unroll
                for (int db = 0; db < DB; ++db)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
                if constexpr (!G::ONES) l_valu *= alpha;
            }
            // P^T = exp(S^T - m) as packed bf16 B operands, then O^T[d][q] += V^T[d][key] P^T[key][q]
#pragma unroll
            for (int k2 = 0; k2 < 2; ++k2) {
                float e[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) e[r] = __builtin_amdgcn_exp2f(sc[k2][r] * LOG2E - mb);
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    uint4 pf;
                    pf.x = pack_bf16(e[8 * s2 + 0], e[8 * s2 + 1]);
                    pf.y = pack_bf16(e[8 * s2 + 2], e[8 * s2 + 3]);
                    pf.z = pack_bf16(e[8 * s2 + 4], e[8 * s2 + 5]);
                    pf.w = pack_bf16(e[8 * s2 + 6], e[8 * s2 + 7]);
                    if constexpr (!G::ONES) {  // the sum of exactly the bf16-rounded probabilities the numerator uses
                        const uint32_t pw[4] = {pf.x, pf.y, pf.z, pf.w};
#pragma unroll
                        for (int q = 0; q < 4; ++q) l_valu += __uint_as_float(pw[q] << 16) + __uint_as_float(pw[q] & 0xffff0000u);
                    }
                    const char* vrow = sV + (k2 * 32 + s2 * 16) * ROW + vbase;
#pragma unroll
                    for (int db = 0; db < DB; ++db) {
                        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                            (__attribute__((address_space(3))) s16x4*)(vrow + db * 64));
                        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                            (__attribute__((address_space(3))) s16x4*)(vrow + db * 64 + 8 * ROW));
                        uint4 vf = __builtin_bit_cast(uint4, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
                        // rows d = 88..95 of V^T do not exist: feeding ones there makes those output rows the row sum
                        // of exactly the bf16-rounded probabilities the numerator uses -- no v_add chain, no shuffle
                        if (db == DB - 1 && c32 >= HD - 32 * (DB - 1)) vf = ones;
                        o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, vf),
                                                                        __builtin_bit_cast(bf16x8, pf), o[db], 0, 0, 0);
                    }
                }
            }
        }
        float l = (DBG & 2) ? 1.f : o[DB - 1][12];  // row 24 (hh = 0) / 28 (hh = 1) of the last block: "ones" rows
        if constexpr (!G::ONES) l = l_valu + __shfl_xor(l_valu, 32, 64);  // this lane's keys + the other half's
        rl_prev = 1.0f / l;
        pb = b; pw = w; ph = h;
        have_prev = true;
        b = nb; w = nwn; h = nh;
    }
    wait_vm<0>();  // trailing re-loads must not outlive the LDS allocation
    if (!(DBG & 8)) store_o(pb, pw, ph, rl_prev);
}

}  // namespace

int swiftk_launch_attn_pipe(const AttnPipeArgs& a, hipStream_t st) {
    const int nitems = a.B * (a.gh / 16) * (a.gw / 16) * a.heads;
    // one item per CU round is the floor; with fewer items than CUs shrink the grid (every workgroup gets floor or
    // ceil of nitems/grid)
    int grid = 256;
    if (nitems < grid) grid = nitems >= 8 ? (nitems & ~7) : nitems;  // a multiple of 8 keeps the XCD-concurrent order
    if (a.hd == 80 || a.hd == 96) {
        if (a.dbg) return SWIFTK_EINVAL;  // the ablation builds exist for head_dim 88 only
        if (a.hd == 80) hipLaunchKernelGGL((attn_pipe_kernel<0, 80>), dim3(grid), dim3(NT), 0, st, a, nitems);
        else hipLaunchKernelGGL((attn_pipe_kernel<0, 96>), dim3(grid), dim3(NT), 0, st, a, nitems);
        SWIFTK_CHECK_LAUNCH();
        return 0;
    }
    if (a.hd != 88) return SWIFTK_ESHAPE;
    switch (a.dbg) {
        case 0: hipLaunchKernelGGL((attn_pipe_kernel<0, 88>), dim3(grid), dim3(NT), 0, st, a, nitems); break;
        case 1: hipLaunchKernelGGL((attn_pipe_kernel<1, 88>), dim3(grid), dim3(NT), 0, st, a, nitems); break;
        case 2: hipLaunchKernelGGL((attn_pipe_kernel<2, 88>), dim3(grid), dim3(NT), 0, st, a, nitems); break;
        case 5: hipLaunchKernelGGL((attn_pipe_kernel<5, 88>), dim3(grid), dim3(NT), 0, st, a, nitems); break;
        case 8: hipLaunchKernelGGL((attn_pipe_kernel<8, 88>), dim3(grid), dim3(NT), 0, st, a, nitems); break;
        case 13: hipLaunchKernelGGL((attn_pipe_kernel<13, 88>), dim3(grid), dim3(NT), 0, st, a, nitems); break;
        case 14: hipLaunchKernelGGL((attn_pipe_kernel<14, 88>), dim3(grid), dim3(NT), 0, st, a, nitems); break;
        default: return SWIFTK_EINVAL;
    }
    SWIFTK_CHECK_LAUNCH();
    return 0;
}
