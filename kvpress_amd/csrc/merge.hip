// MergingPress.merge (kvpress/presses/merging_press.py:99-177; include/kvpress_hip.h: kvp_merge_values): every evicted token's value is
// folded into the value of the kept token whose key is most cosine-similar, in place in the gathered V'.
//   1. prep: the evicted positions as the ascending complement of the kept set (:124-127), 1 / max(||k||, 1e-6) and ||v|| of every
//      kept row (from K' and V' BEFORE the merge, :155) and every evicted row;
//   2. nearest survivor: argmax_j dot(k_e, k_j) / max(||k_j||, 1e-6) over the kept rows (:137-139) without ever writing the
//      [n_evict, n_kept] similarity matrix -- an MFMA GEMM on the raw 16-bit keys (exact products, fp32 sums) whose epilogue keeps a
//      running (max, index) per evicted row; ties go to the LOWEST index in the kept list (torch's first occurrence); short rows split
//      the kept dimension over workgroups and merge the partial maxima in split order;
//   3. gates and weights (:141-156): threshold, the per-row quantile of the fraction gate with ATen's arithmetic, the value-norm weight;
//   4. merge (:158-173): the contributors of every kept row in ascending evicted position (the order of the CPU reference's
//      scatter_add_), summed in fp32 with separately rounded products and sums; rows with sum(w) > 0 are rewritten, the others untouched.
// No float atomics: integer counts and bucket slots only, and every bucket is replayed in ascending evicted position, so the output is
// bit-identical from run to run.  Workspace: 32 bytes per (b, h, token) plus O(B*H*S/1024) (kvp_merge_workspace_bytes).
#include <math.h>

#include "kvp_mfma.h"

namespace {

constexpr int MT = 256;          // threads of the element-wise kernels
constexpr int TILE = 1024;       // positions per compaction tile
constexpr int SEL_THREADS = 1024;
constexpr int AM_WAVES = 4;      // MFMA argmax: waves per workgroup
constexpr int AM_KT = 64;        // kept rows staged per LDS buffer
constexpr int GN_EV = 32;        // generic argmax: evicted rows per workgroup
constexpr int GN_KT = 16;        // generic argmax: kept rows per LDS tile
constexpr float EPS = 1e-6f;     // merging_press.py:14

// (value, index) of the better candidate: larger value, ties to the lower index; NaN never wins
__device__ __forceinline__ void better(float& bv, int& bi, float v, int i) {
    if (v > bv || (v == bv && (unsigned)i < (unsigned)bi)) {
        bv = v;
        bi = i;
    }
}

// ---- workspace layout (per row r = b * H + h; arrays of S entries per row) -----------------------------------------------------
struct MrgWs {
    int64_t ntile;
    int32_t* ev;    // evicted positions, ascending
    float* inv;     // 1 / max(||k||, eps): [0, n_kept) kept rows (K' order), [n_kept, S) evicted rows
    float* vn;      // ||v||, same layout
    float* ms;      // max_sim [n_evict]
    int32_t* tg;    // target [n_evict]
    float* w;       // weights [n_evict]; before them the argmax partial maxima (P * n_evict <= S)
    int32_t* cnt;   // [S + 1] per row: the kept mask, then counts -> bucket ends per kept row
    int32_t* lst;   // bucket contents; before them the argmax partial indices
    int32_t* tcnt;  // [ntile]
    float* thr;     // one per row
    size_t total;
};
MrgWs mrg_ws(void* ws, int64_t R, int64_t S) {
    MrgWs L;
    L.ntile = (S + TILE - 1) / TILE;
    KvpArena ar(ws);
    const size_t row = (size_t)R * S;
    L.ev = ar.take<int32_t>(row);
    L.inv = ar.take<float>(row);
    L.vn = ar.take<float>(row);
    L.ms = ar.take<float>(row);
    L.tg = ar.take<int32_t>(row);
    L.w = ar.take<float>(row);
    L.cnt = ar.take<int32_t>((size_t)R * (S + 1));
    L.lst = ar.take<int32_t>(row);
    L.tcnt = ar.take<int32_t>((size_t)R * L.ntile);
    L.thr = ar.take<float>((size_t)R);
    L.total = ar.bytes();
    return L;
}

// ---- 1. prep ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MT) void mrg_mark_kernel(const int32_t* __restrict__ kept, int64_t nk, int64_t S, int32_t* __restrict__ cnt) {
    const int64_t r = blockIdx.y;
    const int64_t j = (int64_t)blockIdx.x * MT + threadIdx.x;
    if (j < nk) {
        const int32_t p = kept[r * nk + j];
        if (p >= 0 && p < S) cnt[r * (S + 1) + p] = 1;
    }
}

__global__ __launch_bounds__(MT) void mrg_tile_count_kernel(const int32_t* __restrict__ cnt, int64_t S, int64_t ntile, int32_t* __restrict__ tcnt) {
    __shared__ int red[MT / 64];
    const int64_t r = blockIdx.y, t = blockIdx.x;
    int c = 0;
    for (int i = threadIdx.x; i < TILE; i += MT) {
        const int64_t s = t * TILE + i;
        if (s < S && cnt[r * (S + 1) + s] == 0) ++c;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);   // (written out: through a wave_sum call the scheduler moves the wave-index shift below)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int i = 0; i < MT / 64; ++i) s += red[i];
        tcnt[r * ntile + t] = s;
    }
}

// block-wide exclusive scan of one int per thread (MT threads); returns the thread's offset, *total the block sum
__device__ __forceinline__ int block_excl_scan(int v, int* sh, int* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    __syncthreads();
    if (lane == 63) sh[w] = x;
    __syncthreads();
    int base = 0, tot = 0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) {
        if (i < w) base += sh[i];
        tot += sh[i];
    }
    *total = tot;
    return base + x - v;
}

__global__ __launch_bounds__(MT) void mrg_compact_kernel(const int32_t* __restrict__ cnt, int64_t S, int64_t ntile, const int32_t* __restrict__ tcnt,
                                                         int64_t ne, int32_t* __restrict__ ev) {
    __shared__ int sh[MT / 64];
    const int64_t r = blockIdx.y, t = blockIdx.x;
    int base = 0;
    for (int64_t i = 0; i < t; ++i) base += tcnt[r * ntile + i];
    constexpr int PER = TILE / MT;
    const int64_t s0 = t * TILE + (int64_t)threadIdx.x * PER;
    int f[PER], c = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        f[i] = (s0 + i < S && cnt[r * (S + 1) + s0 + i] == 0) ? 1 : 0;
        c += f[i];
    }
    int tot;
    int o = base + block_excl_scan(c, sh, &tot);
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        if (f[i]) {
            if (o < ne) ev[r * S + o] = (int32_t)(s0 + i);
            ++o;
        }
    }
}

// one wave per (row, slot): slot < nk -> kept row slot of K' / V', else evicted row slot - nk of the cache
template <int DT>
__global__ __launch_bounds__(MT) void mrg_norms_kernel(const typename Elem<DT>::T* __restrict__ k, int64_t k_sb, int64_t k_sh, int64_t k_ss,
                                                       const typename Elem<DT>::T* __restrict__ v, int64_t v_sb, int64_t v_sh, int64_t v_ss,
                                                       const typename Elem<DT>::T* __restrict__ ko, const typename Elem<DT>::T* __restrict__ vo,
                                                       int H, int64_t S, int64_t nk, int D, const int32_t* __restrict__ ev,
                                                       float* __restrict__ inv, float* __restrict__ vn) {
    using T = typename Elem<DT>::T;
    const int64_t r = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * (MT / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= S) return;
    const T *kr, *vr;
    if (i < nk) {
        kr = ko + (r * nk + i) * D;
        vr = vo + (r * nk + i) * D;
    } else {
        const int64_t b = r / H, h = r % H, p = ev[r * S + (i - nk)];
        kr = k + b * k_sb + h * k_sh + p * k_ss;
        vr = v + b * v_sb + h * v_sh + p * v_ss;
    }
    float sk = 0.f, sv = 0.f;
    for (int d = lane; d < D; d += 64) {
        const float a = Elem<DT>::ld(kr + d), c = Elem<DT>::ld(vr + d);
        sk = fmaf(a, a, sk);
        sv = fmaf(c, c, sv);
    }
    sk = wave_sum(sk);
    sv = wave_sum(sv);
    if (lane == 0) {
        inv[r * S + i] = 1.f / fmaxf(sqrtf(sk), EPS);
        vn[r * S + i] = sqrtf(sv);
    }
}

// ---- 2a. nearest survivor on the matrix cores: bf16 / f16, D in {64, 96, 128, 256}, 16-byte aligned rows ----------------------------
// Workgroup = (block of evicted rows, split of the kept rows, row r); 4 waves, each owning NB x 32 evicted rows whose keys stay in its
// registers (B operand, gathered once through the evicted list).  The kept rows of K' stream through LDS, 64 rows per buffer (16-byte
// chunks XOR-swizzled by row, next buffer prefetched into registers during the MFMAs).  acc = K'_tile x K_e^T: a lane owns one evicted
// column and 16 kept rows, ascending in i, so a strict > keeps the lowest kept index per lane; the two lane halves are merged at the end.
template <int D> struct AmGeo {
    static constexpr int CH = D / 8;                                    // 16-byte chunks per row
    static constexpr int KS = D / 16;                                   // MFMA k-steps
    static constexpr int NB = D <= 128 ? 2 : 1;                         // 32-column blocks per wave
    static constexpr int EVB = AM_WAVES * 32 * NB;                      // evicted rows per workgroup
    static constexpr int LD = (AM_KT * CH + AM_WAVES * 64 - 1) / (AM_WAVES * 64);   // 16-byte loads per thread per buffer
    static __device__ __forceinline__ int swz(int r, int c) { return c ^ (r & ((D % 128 == 0 || D == 64) ? 7 : 3)); }
};

template <int DT, int D>
__global__ __launch_bounds__(AM_WAVES * 64) void mrg_argmax_mfma_kernel(
    const typename Elem<DT>::T* __restrict__ k, int64_t k_sb, int64_t k_sh, int64_t k_ss, const typename Elem<DT>::T* __restrict__ ko,
    int H, int64_t S, int64_t nk, int64_t ne, int64_t kchunk, const int32_t* __restrict__ ev, const float* __restrict__ inv,
    float* __restrict__ pval, int32_t* __restrict__ pidx) {
    using G = AmGeo<D>;
    using T = typename Elem<DT>::T;
    __shared__ __attribute__((aligned(16))) uint16_t ks[AM_KT * D];
    __shared__ float invs[AM_KT];
    const int64_t r = blockIdx.z;
    const int p = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r32 = lane & 31, h = lane >> 5;
    const int64_t b = r / H, hh = r % H;
    const int64_t k0 = (int64_t)p * kchunk, k1 = min(nk, k0 + kchunk);

    // evicted operand: NB blocks of 32 columns, gathered through the evicted list
    uint4 bq[G::NB][G::KS];
#pragma unroll
    for (int nb = 0; nb < G::NB; ++nb) {
        const int64_t e = (int64_t)blockIdx.x * G::EVB + (wave * G::NB + nb) * 32 + r32;
        const T* kr = nullptr;
        if (e < ne) kr = k + b * k_sb + hh * k_sh + (int64_t)ev[r * S + e] * k_ss;
#pragma unroll
        for (int s = 0; s < G::KS; ++s) bq[nb][s] = kr ? *reinterpret_cast<const uint4*>(kr + 16 * s + 8 * h) : make_uint4(0, 0, 0, 0);
    }
    float bv[G::NB];
    int bi[G::NB];
#pragma unroll
    for (int nb = 0; nb < G::NB; ++nb) {
        bv[nb] = -INFINITY;
        bi[nb] = -1;
    }
    const T* kb = ko + r * nk * D;
    uint4 pre[G::LD];
    float pinv = 0.f;
    auto fetch = [&](int64_t t0) {
#pragma unroll
        for (int l = 0; l < G::LD; ++l) {
            const int c = threadIdx.x + l * AM_WAVES * 64;
            const int row = c / G::CH, ch = c % G::CH;
            pre[l] = make_uint4(0, 0, 0, 0);
            if (row < AM_KT && t0 + row < k1) pre[l] = *reinterpret_cast<const uint4*>(kb + (t0 + row) * D + ch * 8);
        }
        if (threadIdx.x < AM_KT) pinv = (t0 + threadIdx.x < k1) ? inv[r * S + t0 + threadIdx.x] : __builtin_nanf("");
    };
    if (k0 < k1) fetch(k0);
    for (int64_t t0 = k0; t0 < k1; t0 += AM_KT) {
        __syncthreads();   // the previous tile's MFMAs are done with ks
#pragma unroll
        for (int l = 0; l < G::LD; ++l) {
            const int c = threadIdx.x + l * AM_WAVES * 64;
            const int row = c / G::CH, ch = c % G::CH;
            if (row < AM_KT) *reinterpret_cast<uint4*>(&ks[row * D + G::swz(row, ch) * 8]) = pre[l];
        }
        if (threadIdx.x < AM_KT) invs[threadIdx.x] = pinv;
        __syncthreads();
        if (t0 + AM_KT < k1) fetch(t0 + AM_KT);
#pragma unroll
        for (int sub = 0; sub < AM_KT / 32; ++sub) {
            if (t0 + sub * 32 >= k1) break;
            const int row = sub * 32 + r32;
            f32x16 acc[G::NB];
#pragma unroll
            for (int nb = 0; nb < G::NB; ++nb)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[nb][i] = 0.f;
#pragma unroll
            for (int s = 0; s < G::KS; ++s) {
                const uint4 a = *reinterpret_cast<const uint4*>(&ks[row * D + G::swz(row, 2 * s + h) * 8]);
#pragma unroll
                for (int nb = 0; nb < G::NB; ++nb) acc[nb] = mma32<DT>(a, bq[nb][s], acc[nb]);
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int kr = sub * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;   // the accumulator's row (kept row within the buffer)
                const float iv = invs[kr];
#pragma unroll
                for (int nb = 0; nb < G::NB; ++nb) {
                    const float x = acc[nb][i] * iv;
                    if (x > bv[nb]) {
                        bv[nb] = x;
                        bi[nb] = (int)(t0 + kr);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int nb = 0; nb < G::NB; ++nb) {
        const float ov = __shfl_xor(bv[nb], 32);
        const int oi = __shfl_xor(bi[nb], 32);
        better(bv[nb], bi[nb], ov, oi);
        const int64_t e = (int64_t)blockIdx.x * G::EVB + (wave * G::NB + nb) * 32 + r32;
        if (h == 0 && e < ne) {
            pval[r * S + (int64_t)p * ne + e] = bv[nb];
            pidx[r * S + (int64_t)p * ne + e] = bi[nb];
        }
    }
}

// ---- 2b. nearest survivor, generic: any dtype, D <= 256 (float32 models, other head sizes, unaligned rows) ------------------------
// Workgroup = (32 evicted rows, split, row r), 256 threads: the evicted rows and a tile of 16 kept rows in LDS as float; thread t owns
// evicted row t & 31 and kept rows (t >> 5) + 8 i of each tile; the 8 groups' maxima are merged in group order (ties: lower index).
template <int DT>
__global__ __launch_bounds__(MT) void mrg_argmax_generic_kernel(
    const typename Elem<DT>::T* __restrict__ k, int64_t k_sb, int64_t k_sh, int64_t k_ss, const typename Elem<DT>::T* __restrict__ ko,
    int H, int64_t S, int64_t nk, int64_t ne, int D, int64_t kchunk, const int32_t* __restrict__ ev, const float* __restrict__ inv,
    float* __restrict__ pval, int32_t* __restrict__ pidx) {
    extern __shared__ float gsm[];
    float* es = gsm;                        // [GN_EV][D + 1]
    float* kt = gsm + GN_EV * (D + 1);      // [GN_KT][D]
    float* ki = kt + GN_KT * D;             // [GN_KT]
    __shared__ float rv[MT];
    __shared__ int ri[MT];
    const int64_t r = blockIdx.z;
    const int p = blockIdx.y;
    const int64_t b = r / H, hh = r % H;
    const int64_t e0 = (int64_t)blockIdx.x * GN_EV;
    const int64_t k0 = (int64_t)p * kchunk, k1 = min(nk, k0 + kchunk);
    for (int c = threadIdx.x; c < GN_EV * D; c += MT) {
        const int er = c / D, d = c % D;
        float x = 0.f;
        if (e0 + er < ne) x = Elem<DT>::ld(k + b * k_sb + hh * k_sh + (int64_t)ev[r * S + e0 + er] * k_ss + d);
        es[er * (D + 1) + d] = x;
    }
    const int er = threadIdx.x & (GN_EV - 1), g = threadIdx.x / GN_EV;
    float bv = -INFINITY;
    int bi = -1;
    for (int64_t t0 = k0; t0 < k1; t0 += GN_KT) {
        __syncthreads();
        for (int c = threadIdx.x; c < GN_KT * D; c += MT) {
            const int row = c / D, d = c % D;
            kt[c] = (t0 + row < k1) ? Elem<DT>::ld(ko + (r * nk + t0 + row) * D + d) : 0.f;
        }
        if (threadIdx.x < GN_KT) ki[threadIdx.x] = (t0 + threadIdx.x < k1) ? inv[r * S + t0 + threadIdx.x] : __builtin_nanf("");
        __syncthreads();
        float a0 = 0.f, a1 = 0.f;
        const float* er_ = es + er * (D + 1);
        const float* k0_ = kt + g * D;
        const float* k1_ = kt + (g + 8) * D;
        for (int d = 0; d < D; ++d) {
            const float x = er_[d];
            a0 = fmaf(x, k0_[d], a0);
            a1 = fmaf(x, k1_[d], a1);
        }
        const float x0 = a0 * ki[g], x1 = a1 * ki[g + 8];
        if (x0 > bv) { bv = x0; bi = (int)(t0 + g); }
        if (x1 > bv) { bv = x1; bi = (int)(t0 + g + 8); }
    }
    rv[threadIdx.x] = bv;
    ri[threadIdx.x] = bi;
    __syncthreads();
    if (g == 0 && e0 + er < ne) {
        for (int q = 1; q < MT / GN_EV; ++q) better(bv, bi, rv[q * GN_EV + er], ri[q * GN_EV + er]);
        pval[r * S + (int64_t)p * ne + e0 + er] = bv;
        pidx[r * S + (int64_t)p * ne + e0 + er] = bi;
    }
}

// the splits' maxima in split order (ascending kept ranges: a strict > keeps the lowest index), times 1 / ||k_e||
__global__ __launch_bounds__(MT) void mrg_finalize_kernel(const float* __restrict__ pval, const int32_t* __restrict__ pidx, int P, int64_t S,
                                                          int64_t nk, int64_t ne, const float* __restrict__ inv, float* __restrict__ ms,
                                                          int32_t* __restrict__ tg, float* __restrict__ ms_out, int32_t* __restrict__ tg_out) {
    const int64_t r = blockIdx.y;
    const int64_t e = (int64_t)blockIdx.x * MT + threadIdx.x;
    if (e >= ne) return;
    float bv = pval[r * S + e];
    int bi = pidx[r * S + e];
    for (int p = 1; p < P; ++p) {
        const float v = pval[r * S + (int64_t)p * ne + e];
        if (v > bv) {
            bv = v;
            bi = pidx[r * S + (int64_t)p * ne + e];
        }
    }
    if (bi < 0 || bi >= nk) bi = 0;   // only NaN similarities leave no candidate (torch's max would return a NaN's index)
    const float m = bv * inv[r * S + nk + e];
    ms[r * S + e] = m;
    tg[r * S + e] = bi;
    if (ms_out) ms_out[r * ne + e] = m;
    if (tg_out) tg_out[r * ne + e] = bi;
}

// ---- 3. gates and weights ----------------------------------------------------------------------------------------------------------
// k-th smallest (0-based) of a row of order keys by an MSB-first radix select (4 x 8 bits); every thread gets it
__device__ uint32_t radix_select(const float* __restrict__ x, int64_t n, float thr, int64_t kth, int* hist, uint32_t* res) {
    uint32_t prefix = 0, mask = 0;
    int64_t k = kth;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = threadIdx.x; i < 256; i += SEL_THREADS) hist[i] = 0;
        __syncthreads();
        for (int64_t i = threadIdx.x; i < n; i += SEL_THREADS) {
            const float m = x[i];
            const uint32_t key = float_to_key(m >= thr ? m : -INFINITY);   // gate failures sink to -inf (:147-148)
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255], 1);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int64_t c = 0;
            int d = 0;
            for (; d < 255; ++d) {
                if (c + hist[d] > k) break;
                c += hist[d];
            }
            res[0] = (uint32_t)d;
            res[1] = (uint32_t)(k - c);
        }
        __syncthreads();
        prefix |= res[0] << shift;
        mask |= 255u << shift;
        k = res[1];
        __syncthreads();
    }
    return prefix;
}

// torch.quantile(q, dim=-1) of max_sim.masked_fill(~ok, -inf) per row (:146-150): rank = q * (n - 1) in float32, the floor and ceil
// order statistics, lerp as ATen evaluates it -- NaN when the lower statistic is -inf and the weight < 0.5 (or both are -inf)
__global__ __launch_bounds__(SEL_THREADS) void mrg_quantile_kernel(const float* __restrict__ ms, int64_t S, int64_t ne, float thr, float q,
                                                                   float* __restrict__ qthr) {
    __shared__ int hist[256];
    __shared__ uint32_t res[2];
    const int64_t r = blockIdx.x;
    const float rank = __fmul_rn(q, (float)(ne - 1));
    const int64_t lo = (int64_t)rank;
    const int64_t hi = (int64_t)ceilf(rank);
    const float wgt = __fsub_rn(rank, (float)lo);
    const float a = key_to_float(radix_select(ms + r * S, ne, thr, lo, hist, res));
    const float c = hi == lo ? a : key_to_float(radix_select(ms + r * S, ne, thr, hi, hist, res));
    if (threadIdx.x == 0) {
        const float d = __fsub_rn(c, a);
        qthr[r] = fabsf(wgt) < 0.5f ? __fadd_rn(a, __fmul_rn(wgt, d)) : __fsub_rn(c, __fmul_rn(d, __fsub_rn(1.f, wgt)));
    }
}

// w = clamp(max_sim, 0) * ok * en / (en + tn + eps) (:141-156), evaluated left to right in float32; contributors are counted per target
__global__ __launch_bounds__(MT) void mrg_weight_kernel(const float* __restrict__ ms, const int32_t* __restrict__ tg, const float* __restrict__ vn,
                                                        const float* __restrict__ qthr, int64_t S, int64_t nk, int64_t ne, float thr,
                                                        float* __restrict__ w, int32_t* __restrict__ cnt) {
    const int64_t r = blockIdx.y;
    const int64_t e = (int64_t)blockIdx.x * MT + threadIdx.x;
    if (e >= ne) return;
    const float m = ms[r * S + e];
    const int t = tg[r * S + e];
    bool ok = m >= thr;
    if (qthr) ok = ok && (m >= qthr[r]);
    const float en = vn[r * S + nk + e], tn = vn[r * S + t];
    const float w0 = __fmul_rn(fmaxf(m, 0.f), ok ? 1.f : 0.f);
    const float x = __fmul_rn(w0, en) / __fadd_rn(__fadd_rn(en, tn), EPS);
    w[r * S + e] = x;
    if (x > 0.f) atomicAdd(&cnt[r * (S + 1) + t], 1);
}

// exclusive scan of the per-target counts of each row, in place (one workgroup per row)
__global__ __launch_bounds__(MT) void mrg_scan_kernel(int32_t* __restrict__ cnt, int64_t S, int64_t nk) {
    __shared__ int sh[MT / 64];
    int32_t* c = cnt + blockIdx.x * (S + 1);
    int base = 0;
    for (int64_t j0 = 0; j0 < nk; j0 += MT) {
        const int64_t j = j0 + threadIdx.x;
        const int v = j < nk ? c[j] : 0;
        int tot;
        const int o = block_excl_scan(v, sh, &tot);
        if (j < nk) c[j] = base + o;
        base += tot;
    }
}

// bucket slots (their order within a bucket is arbitrary; the merge replays every bucket in ascending evicted position)
__global__ __launch_bounds__(MT) void mrg_fill_kernel(const int32_t* __restrict__ tg, const float* __restrict__ w, int64_t S, int64_t ne,
                                                      int32_t* __restrict__ cnt, int32_t* __restrict__ lst) {
    const int64_t r = blockIdx.y;
    const int64_t e = (int64_t)blockIdx.x * MT + threadIdx.x;
    if (e >= ne || !(w[r * S + e] > 0.f)) return;
    const int slot = atomicAdd(&cnt[r * (S + 1) + tg[r * S + e]], 1);
    lst[r * S + slot] = (int32_t)e;
}

// ---- 4. merge: one wave per kept row ---------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(MT) void mrg_merge_kernel(const typename Elem<DT>::T* __restrict__ v, int64_t v_sb, int64_t v_sh, int64_t v_ss,
                                                       typename Elem<DT>::T* __restrict__ vo, int H, int64_t S, int64_t nk, int64_t ne, int D,
                                                       const int32_t* __restrict__ ev, const int32_t* __restrict__ tg,
                                                       const float* __restrict__ w, const int32_t* __restrict__ cnt,
                                                       const int32_t* __restrict__ lst) {
    using T = typename Elem<DT>::T;
    const int64_t r = blockIdx.y;
    const int64_t j = (int64_t)blockIdx.x * (MT / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (j >= nk) return;
    const int32_t* c = cnt + r * (S + 1);
    const int lo = j ? c[j - 1] : 0, hi = c[j];
    const int m = hi - lo;
    if (m <= 0) return;   // no contribution: the row stays as gathered (:169-173)
    const int64_t b = r / H, hh = r % H;
    const T* vb = v + b * v_sb + hh * v_sh;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    float ws = 0.f;
    auto add = [&](int64_t e) {
        const float we = w[r * S + e];
        const T* vr = vb + (int64_t)ev[r * S + e] * v_ss;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int d = lane + 64 * q;
            if (d < D) acc[q] = __fadd_rn(acc[q], __fmul_rn(we, Elem<DT>::ld(vr + d)));
        }
        ws = __fadd_rn(ws, we);
    };
    if (m <= 64) {
        // a bucket of at most 64 entries: rank them in the wave (distinct evicted indices), replay in ascending order
        const int me = lane < m ? lst[r * S + lo + lane] : 0x7FFFFFFF;
        int rank = 0;
        for (int i = 0; i < m; ++i) rank += (__shfl(me, i) < me) ? 1 : 0;
        for (int i = 0; i < m; ++i) {
            const uint64_t bal = __ballot(lane < m && rank == i);
            const int src = __ffsll((unsigned long long)bal) - 1;
            add(__shfl(me, src));
        }
    } else {
        // a large bucket: walk the row's evicted tokens in ascending order and take those that target j
        for (int64_t e0 = 0; e0 < ne; e0 += 64) {
            const int64_t e = e0 + lane;
            const bool hit = e < ne && tg[r * S + e] == j && w[r * S + e] > 0.f;
            uint64_t bal = __ballot(hit);
            while (bal) {
                const int src = __ffsll((unsigned long long)bal) - 1;
                bal &= bal - 1;
                add(e0 + src);
            }
        }
    }
    if (!(ws > 0.f)) return;
    const float den = __fadd_rn(1.f, ws);
    T* orow = vo + (r * nk + j) * D;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int d = lane + 64 * q;
        if (d < D) orow[d] = to_dt_acc<DT>(__fadd_rn(Elem<DT>::ld(orow + d), acc[q]) / den);   // (integer rounding: the form this kernel was compiled with, no MFMA involved)
    }
}

bool mfma_ok(int dtype, int64_t D, KvpRows k, const void* ko) {
    if (dtype == KVP_F32 || !(D == 64 || D == 96 || D == 128 || D == 256)) return false;
    return k.aligned(16, 2) && ((uintptr_t)ko % 16) == 0;
}

template <int DT>
int mrg_run(const MrgWs& L, hipStream_t st, KvpRows k, KvpRows v, const int32_t* kept, const void* ko, void* vo, int64_t B, int64_t H, int64_t S,
            int64_t nk, int64_t D, float thr, float q, bool frac, int32_t* tg_out, float* ms_out) {
    using T = typename Elem<DT>::T;
    const int64_t R = B * H, ne = S - nk;
    int32_t *const ev = L.ev, *const tg = L.tg, *const cnt = L.cnt, *const lst = L.lst, *const tcnt = L.tcnt;
    float *const inv = L.inv, *const vn = L.vn, *const ms = L.ms, *const w = L.w, *const qthr = L.thr;
    const size_t cnt_bytes = (size_t)R * (S + 1) * 4;

    // 1. prep
    if (hipMemsetAsync(cnt, 0, cnt_bytes, st) != hipSuccess) {
        kvp_set_error("kvp_merge_values: hipMemsetAsync failed");
        return KVP_EHIP;
    }
    KVP_LAUNCH("merge_mark", st, mrg_mark_kernel<<<dim3((unsigned)((nk + MT - 1) / MT), (unsigned)R), MT, 0, st>>>(kept, nk, S, cnt));
    KVP_LAUNCH("merge_tile_count", st, mrg_tile_count_kernel<<<dim3((unsigned)L.ntile, (unsigned)R), MT, 0, st>>>(cnt, S, L.ntile, tcnt));
    KVP_LAUNCH("merge_compact", st, mrg_compact_kernel<<<dim3((unsigned)L.ntile, (unsigned)R), MT, 0, st>>>(cnt, S, L.ntile, tcnt, ne, ev));
    KVP_LAUNCH("merge_norms", st,
               mrg_norms_kernel<DT><<<dim3((unsigned)((S + MT / 64 - 1) / (MT / 64)), (unsigned)R), MT, 0, st>>>(
                   (const T*)k.p, k.sb, k.sh, k.ss, (const T*)v.p, v.sb, v.sh, v.ss, (const T*)ko, (const T*)vo, (int)H, S, nk, (int)D, ev, inv, vn));
    KVP_CHECK_LAUNCH("merge prep");

    // 2. nearest survivor: split the kept rows when the evicted rows alone give fewer than ~2 workgroups per CU (P * ne <= S keeps
    // the partial maxima inside the weight / bucket arrays)
    const bool mf = mfma_ok(DT, D, k, ko);   // false for float32
    int evb = GN_EV, kgran = GN_KT;
    if (mf) {
        evb = D <= 128 ? AmGeo<128>::EVB : AmGeo<256>::EVB;
        kgran = AM_KT;
    }
    const int64_t nxb = (ne + evb - 1) / evb;
    const int64_t ktiles = (nk + kgran - 1) / kgran;
    int64_t P = std::max<int64_t>(1, std::min<int64_t>({(512 + nxb * R - 1) / (nxb * R), ktiles, S / ne, (int64_t)16}));
    const int64_t kchunk = ((ktiles + P - 1) / P) * kgran;
    P = (nk + kchunk - 1) / kchunk;
    const dim3 ag((unsigned)nxb, (unsigned)P, (unsigned)R);
    float* pval = w;
    int32_t* pidx = lst;
    if constexpr (DT != KVP_F32) {
      if (mf) {
        switch (D) {
#define MRG_AM(D_) \
    case D_: KVP_LAUNCH("merge_argmax_mfma", st, mrg_argmax_mfma_kernel<DT, D_><<<ag, AM_WAVES * 64, 0, st>>>((const T*)k.p, k.sb, k.sh, k.ss, (const T*)ko, (int)H, S, nk, ne, kchunk, ev, inv, pval, pidx)); break;
            MRG_AM(64)
            MRG_AM(96)
            MRG_AM(128)
            MRG_AM(256)
#undef MRG_AM
        }
        KVP_CHECK_LAUNCH("mrg_argmax_mfma_kernel");
      }
    }
    if (!mf) {
        const size_t lds = (size_t)(GN_EV * (D + 1) + GN_KT * D + GN_KT) * sizeof(float);
        KVP_LAUNCH("merge_argmax_generic", st,
                   mrg_argmax_generic_kernel<DT><<<ag, MT, lds, st>>>((const T*)k.p, k.sb, k.sh, k.ss, (const T*)ko, (int)H, S, nk, ne, (int)D, kchunk,
                                                                      ev, inv, pval, pidx));
        KVP_CHECK_LAUNCH("mrg_argmax_generic_kernel");
    }
    const dim3 eg((unsigned)((ne + MT - 1) / MT), (unsigned)R);
    KVP_LAUNCH("merge_finalize", st, mrg_finalize_kernel<<<eg, MT, 0, st>>>(pval, pidx, (int)P, S, nk, ne, inv, ms, tg, ms_out, tg_out));

    // 3. gates and weights; the kept mask in cnt becomes the per-target counts
    if (frac) KVP_LAUNCH("merge_quantile", st, mrg_quantile_kernel<<<(unsigned)R, SEL_THREADS, 0, st>>>(ms, S, ne, thr, q, qthr));
    if (hipMemsetAsync(cnt, 0, cnt_bytes, st) != hipSuccess) {
        kvp_set_error("kvp_merge_values: hipMemsetAsync failed");
        return KVP_EHIP;
    }
    KVP_LAUNCH("merge_weight", st, mrg_weight_kernel<<<eg, MT, 0, st>>>(ms, tg, vn, frac ? qthr : nullptr, S, nk, ne, thr, w, cnt));
    // 4. buckets and merge
    KVP_LAUNCH("merge_scan", st, mrg_scan_kernel<<<(unsigned)R, MT, 0, st>>>(cnt, S, nk));
    KVP_LAUNCH("merge_fill", st, mrg_fill_kernel<<<eg, MT, 0, st>>>(tg, w, S, ne, cnt, lst));
    KVP_LAUNCH("merge_values", st,
               mrg_merge_kernel<DT><<<dim3((unsigned)((nk + MT / 64 - 1) / (MT / 64)), (unsigned)R), MT, 0, st>>>(
                   (const T*)v.p, v.sb, v.sh, v.ss, (T*)vo, (int)H, S, nk, ne, (int)D, ev, tg, w, cnt, lst));
    KVP_CHECK_LAUNCH("merge");
    return KVP_OK;
}

}  // namespace

// ================================================================================================================================
extern "C" size_t kvp_merge_workspace_bytes(int64_t B, int64_t H, int64_t S, int64_t n_kept, int64_t D) {
    (void)D;
    if (B < 1 || H < 1 || S < 1 || n_kept < 0 || n_kept > S) return 0;
    return mrg_ws(nullptr, B * H, S).total;
}

extern "C" int kvp_merge_values(const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss, const void* v, int64_t v_sb, int64_t v_sh,
                                int64_t v_ss, const int32_t* kept_idx, const void* k_out, void* v_out, int dtype, int64_t B, int64_t H,
                                int64_t S, int64_t n_kept, int64_t D, double similarity_threshold, double merge_fraction, void* ws,
                                size_t ws_bytes, int32_t* target, float* max_sim, kvp_stream_t stream) {
    KVP_CHECK_DTYPE("kvp_merge_values", dtype);
    KVP_CHECK_ARG(B >= 1 && H >= 1 && S >= 1 && D >= 1 && n_kept >= 0 && n_kept <= S, "kvp_merge_values: bad shape");
    KVP_CHECK_ARG(S < ((int64_t)1 << 31) / 2 && B * H < 65536, "kvp_merge_values: bad shape (S, B * H too large)");
    KVP_CHECK_ARG(D <= 256, "kvp_merge_values: head size %lld > 256 is not supported", (long long)D);
    KVP_CHECK_ARG(merge_fraction > 0.0 && merge_fraction <= 1.0, "kvp_merge_values: merge_fraction must be in (0, 1]");
    const int64_t ne = S - n_kept;
    if (ne == 0 || n_kept == 0) return KVP_OK;   // merging_press.py:120-121: nothing to merge
    KVP_CHECK_ARG(k && v && kept_idx && k_out && v_out && ws, "kvp_merge_values: null pointer");
    const MrgWs L = mrg_ws(ws, B * H, S);
    if (int rc = kvp_check_workspace("kvp_merge_values", ws, ws_bytes, L.total)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const float thr = (float)similarity_threshold;          // `max_sim >= threshold` compares in float32
    const float q = (float)(1.0 - merge_fraction);          // torch.quantile's q tensor has the input's dtype
    const bool frac = merge_fraction < 1.0;
    KVP_DISPATCH_DTYPE(dtype, return mrg_run<DT>(L, st, {k, k_sb, k_sh, k_ss}, {v, v_sb, v_sh, v_ss}, kept_idx, k_out, v_out, B, H, S, n_kept, D, thr, q, frac, target, max_sim));
}
