// KVzip's scorer (kvpress/presses/kvzip_press.py:312-354; include/kvpress_hip.h: kvp_kvzip_score): the maximum, over the query heads of a
// kv head and over the rows of the "repeat the context" forward, of the attention every row pays to the keys of one context chunk,
//     out[b,h,j] = max_{g<G, t<Lq} softmax_{V(t)}(q_{g,t} . k / sqrt(D))[j] * row_scale[t] * col_scale[hG+g, j],    j in [start, end)
//     V(t) = [0, sink) u [start, end) u {S - Lq + u : u <= t}      (sink keys, the chunk, the causal part of the repeated rows).
// The reference concatenates the three key ranges, stores the whole [Hkv, G, Lq, sink + ctx + Lq] softmax, masks it, slices it and takes
// the amax.  Here nothing with an Lq x keys extent exists.  Two passes over the logits, both on one kernel shape: a workgroup OWNS a block of
// rows of one operand in registers (the MFMA's B operand) and STREAMS the rows of the other through LDS (A operand, kvp_mfma.h's swizzled
// tile filled by LDS-DMA, double-buffered), so a lane's 16 accumulators are 16 streamed rows against ONE owned row and both reductions
// run inside the lane:
//   pass 1 owns query rows, streams the keys of V(t) (tiles wholly above the causal diagonal are never requested) and keeps the running
//          (max, sum) of every row; the key range is split over workgroups and the partials are folded by kz_combine_kernel into
//          lse = max + log2(sum) per row;
//   pass 2 owns chunk keys, streams the query rows of one head and keeps max_t 2^(logit - lse[t]) * row_scale[t] per key; rows and heads
//          are split over workgroups, and the partial maxima are folded by kz_merge_kernel.
// A maximum is exact under any partition and the softmax partials are folded in a fixed order: bit-identical from run to run, no atomics.
// Everything works in log2 units (softmax_stats.h).  row_scale and col_scale are norms (>= 0): the column factor is applied once per key.
#include <math.h>

#include <type_traits>

#include "kvp_mfma.h"
#include "softmax_stats.h"

namespace {

constexpr int KZ_THREADS = 256;   // 4 waves
constexpr int KZ_PAD = 128;       // lse / row-scale rows are padded to a multiple of the longest streamed tile
constexpr int64_t KZ_UNITS = 1024;   // workgroups a pass is split into when the shape allows (256 CUs, two workgroups each, twice over)

struct KzArgs {
    const void *qrot, *k;         // RoPE'd queries [B,Hq,Lq,D] contiguous in the model dtype; keys [B,Hkv,S,D]
    int64_t k_sb, k_sh, k_ss;
    int Hq, Hkv, G, D;
    int64_t S, Lq, Lqp, sink, start, ctx;
    float c;                      // log2(e) / sqrt(D)
    float *pm, *pz;               // pass-1 partials [nks][B*Hq*Lq] (log2 units)
    float *lse, *rsp;             // [B*Hq][Lqp] (+inf in the padding), [B][Lqp] (0 in the padding)
    const float *rs, *cs;         // row_scale [B,Lq], col_scale [B,Hq,ctx]; either may be null
    float* part;                  // pass-2 partial maxima [nsplit][B*Hkv][ctx]
    float* out;
    int64_t out_stride, nrow, npart;   // nrow = B*Hq*Lq, npart = B*Hkv*ctx
    uint32_t nks, tps, ntt;       // pass 1: key splits, streamed tiles per split, row tiles
    uint32_t nkt, nrs, rps;       // pass 2: key tiles, row splits per head, rows per split
};

// virtual key v of V(t) -> row of the cache
__device__ __forceinline__ int64_t kz_key_row(const KzArgs& a, int64_t v) {
    return v < a.sink ? v : v < a.sink + a.ctx ? a.start + (v - a.sink) : a.S - a.Lq + (v - a.sink - a.ctx);
}

// ---- q_rot = q * cos + rotate_half(q) * sin with torch's per-op rounding (kvzip_press.py:312-313), one thread per (row, d < D/2) -----------
template <int DT>
__global__ __launch_bounds__(KZ_THREADS) void kz_rope_kernel(const typename Elem<DT>::T* __restrict__ q, int64_t q_sb, int64_t q_sh, int64_t q_ss,
                                                             const typename Elem<DT>::T* __restrict__ cosp,
                                                             const typename Elem<DT>::T* __restrict__ sinp, int64_t cs_sb, int64_t cs_sw,
                                                             int64_t B, int64_t Hq, int64_t Lq, int64_t D, typename Elem<DT>::T* __restrict__ out) {
    const int64_t half = D / 2, total = B * Hq * Lq * half;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t d = i % half, row = i / half;
        const int64_t t = row % Lq, bh = row / Lq;
        const int64_t hq = bh % Hq, b = bh / Hq;
        const typename Elem<DT>::T* qr = q + b * q_sb + hq * q_sh + t * q_ss;
        const typename Elem<DT>::T* cr = cosp + b * cs_sb + t * cs_sw;
        const typename Elem<DT>::T* sr = sinp + b * cs_sb + t * cs_sw;
        const float q0 = Elem<DT>::ld(qr + d), q1 = Elem<DT>::ld(qr + d + half);
        typename Elem<DT>::T* o = out + row * D;
        st_dt<DT>(o + d, rope_elem<DT>(q0, Elem<DT>::ld(cr + d), -q1, Elem<DT>::ld(sr + d)));
        st_dt<DT>(o + d + half, rope_elem<DT>(q1, Elem<DT>::ld(cr + d + half), q0, Elem<DT>::ld(sr + d + half)));
    }
}

// ---- matrix-core path: bf16 / f16, D in {64, 96, 128, 256}, 16-byte aligned key rows --------------------------------------------------------
// Geometry (vwl1.hip's): wave w owns NB blocks of 32 rows (256 a workgroup for D <= 128, 128 for D = 256), DK k-steps of uint4 per block,
// loaded once.  A streamed tile is 128 LDS rows; D = 256 puts the two 256-byte halves of a row into two consecutive LDS rows (64 rows a
// tile).  acc = streamed rows x owned rows^T per 32 streamed rows: lane (n, half) holds streamed rows {0..3, 8..11, 16..19, 24..27} + 4 * half
// of owned row n.  Streamed rows past the end are requested clamped to the last row (a skipped request would leave stale LDS behind) and
// drop out by the causal test (pass 1) or by lse = +inf, row_scale = 0 in the padding (pass 2).
template <int D> struct KzGeo : KTileGeo<(D == 256 ? 8 : D / 16), KZ_THREADS> {
    using Base = KTileGeo<(D == 256 ? 8 : D / 16), KZ_THREADS>;
    static constexpr int DK = D / 16;                  // MFMA k-steps of a head
    static constexpr int HALVES = D == 256 ? 2 : 1;    // LDS rows per streamed row
    static constexpr int WT = Base::TILE / HALVES;     // streamed rows per tile
    static constexpr int SUBS = WT / 32;
    static constexpr int NB = D <= 128 ? 2 : 1;        // 32-row blocks per wave
    static constexpr int TOK = (KZ_THREADS / 64) * 32 * NB;
};

template <int DT, int D, int PASS>
__global__ __launch_bounds__(KZ_THREADS, 2) void kvzip_mfma_kernel(KzArgs a) {
    using Geo = KzGeo<D>;
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * Geo::TILEB];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t n = lane & 31, kg = lane >> 5;

    // the unit of this workgroup: what it owns, what it streams
    int64_t own0, nown, own_stride, nstr, str_stride, t_first, t_last, bh;
    const char *ownbase, *strbase;
    uint32_t split = 0, row = 0;
    if (PASS == 1) {
        const uint32_t ks = blockIdx.x % a.nks, u2 = blockIdx.x / a.nks;
        const uint32_t tt = a.ntt - 1 - u2 % a.ntt;   // the longest key ranges first
        bh = u2 / a.ntt;                              // b * Hq + query head
        const int64_t b = bh / a.Hq, hkv = (bh % a.Hq) / a.G;
        own0 = (int64_t)tt * Geo::TOK; nown = a.Lq; own_stride = (int64_t)D * 2;
        ownbase = static_cast<const char*>(a.qrot) + bh * a.Lq * D * 2;
        nstr = a.sink + a.ctx + min(a.Lq, own0 + Geo::TOK);   // the keys the last owned row sees
        str_stride = a.k_ss * 2;
        strbase = static_cast<const char*>(a.k) + (b * a.k_sb + hkv * a.k_sh) * 2;
        t_first = (int64_t)ks * a.tps;
        t_last = min((int64_t)(ks + 1) * a.tps, (nstr + Geo::WT - 1) / Geo::WT);
        split = ks;
    } else {
        const uint32_t kt = blockIdx.x % a.nkt, u2 = blockIdx.x / a.nkt;
        const uint32_t rsp = u2 % a.nrs, u3 = u2 / a.nrs;
        const uint32_t g = u3 % a.G;
        row = u3 / a.G;                               // b * Hkv + kv head
        const int64_t b = row / a.Hkv, h = row % a.Hkv;
        bh = b * a.Hq + h * a.G + g;
        own0 = (int64_t)kt * Geo::TOK; nown = a.ctx; own_stride = a.k_ss * 2;
        ownbase = static_cast<const char*>(a.k) + (b * a.k_sb + h * a.k_sh + a.start * a.k_ss) * 2;
        nstr = a.Lq; str_stride = (int64_t)D * 2;
        strbase = static_cast<const char*>(a.qrot) + bh * a.Lq * D * 2;
        t_first = (int64_t)rsp * a.rps / Geo::WT;
        t_last = (min(a.Lq, (int64_t)(rsp + 1) * a.rps) + Geo::WT - 1) / Geo::WT;
        split = g * a.nrs + rsp;
    }
    const int64_t wown0 = own0 + wv * (32 * Geo::NB);   // first owned row of this wave

    if (PASS == 1 && t_first >= t_last) {   // a key split wholly above the causal diagonal of these rows: the empty partial
#pragma unroll
        for (int nb = 0; nb < Geo::NB; ++nb) {
            const int64_t t = wown0 + nb * 32 + n;
            if (kg == 0 && t < a.Lq) {
                a.pm[(int64_t)split * a.nrow + bh * a.Lq + t] = KVP_NEG_INF;
                a.pz[(int64_t)split * a.nrow + bh * a.Lq + t] = 0.f;
            }
        }
        return;
    }

    // the owned rows (B operand): k-step ks, lane half kg = elements 16 ks + 8 kg .. + 8; rows past the end are zero rows
    uint4 vf[Geo::NB][Geo::DK];
#pragma unroll
    for (int nb = 0; nb < Geo::NB; ++nb) {
        const int64_t s = wown0 + nb * 32 + n;
        const char* vr = ownbase + s * own_stride + kg * 16;
#pragma unroll
        for (int ks = 0; ks < Geo::DK; ++ks) vf[nb][ks] = s < nown ? *reinterpret_cast<const uint4*>(vr + ks * 32) : make_uint4(0, 0, 0, 0);
    }

    const uint32_t ldsbase = KVP_LDS_ADDR(lds);
    const uint32_t rrow = Geo::RPW * wv + lane / Geo::CPR;        // this lane's LDS row inside a request
    const uint32_t rchunk = (lane % Geo::CPR) ^ Geo::sw(rrow);    // (a request's first row is a multiple of the swizzle period)
    auto request_tile = [&](int64_t t, uint32_t buf_off) {
#pragma unroll
        for (int j = 0; j < Geo::NREQ; ++j) {
            const uint32_t lr = Geo::RPR * j + rrow;
            const int64_t sr = min(t * Geo::WT + lr / Geo::HALVES, nstr - 1);   // rows past the end: the last row (dropped below)
            const char* gp = strbase + (PASS == 1 ? kz_key_row(a, sr) : sr) * str_stride + (lr % Geo::HALVES) * 256 + (rchunk << 4);
            const uint32_t la = __builtin_amdgcn_readfirstlane(ldsbase + buf_off + (Geo::RPR * j + Geo::RPW * wv) * Geo::ROWB);
            if (Geo::NCH == Geo::CPR) lds_dma16(la, gp);
            else lds_dma16_if(rchunk < (uint32_t)Geo::NCH, la, gp);
        }
    };
    request_tile(t_first, 0);

    float m[Geo::NB], z[Geo::NB];   // pass 1: running max (raw logits) and sum; pass 2: m = running maximum of the scaled probabilities
#pragma unroll
    for (int nb = 0; nb < Geo::NB; ++nb) { m[nb] = PASS == 1 ? KVP_NEG_INF : 0.f; z[nb] = 0.f; }
    const float* lsep = a.lse + bh * a.Lqp;
    const float* rspp = a.rsp + (bh / a.Hq) * a.Lqp;
    const int64_t diag = a.sink + a.ctx;   // virtual key diag + u is row u of the repeated part

    // one tile: per 32 streamed rows DK x NB MFMAs on fresh accumulators, then the lane-local reduction (MASK: the causal test, pass 1)
    auto tile_body = [&](auto mask_tag, int64_t s0, uint32_t buf) {
        constexpr bool MASK = decltype(mask_tag)::value;
#pragma unroll(PASS == 1 ? 2 : Geo::SUBS)   // pass 1 keeps (max, sum) and sixteen logits per block live: unrolled over all four sub-tiles it spills at D = 128
        for (int sub = 0; sub < Geo::SUBS; ++sub) {
            f32x16 acc[Geo::NB];
#pragma unroll
            for (int nb = 0; nb < Geo::NB; ++nb)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[nb][i] = 0.f;
#pragma unroll
            for (int ks = 0; ks < Geo::DK; ++ks) {
                const uint32_t ch = ks * 2 + kg;                                                       // 16-byte chunk of the streamed row
                const uint32_t lr = (sub * 32 + n) * Geo::HALVES + (Geo::HALVES == 2 ? ch >> 4 : 0);   // its LDS row
                const uint4 wf = *reinterpret_cast<const uint4*>(lds + buf + lr * Geo::ROWB + (((ch & (Geo::CPR - 1)) ^ Geo::sw(lr)) << 4));
#pragma unroll
                for (int nb = 0; nb < Geo::NB; ++nb) acc[nb] = mma32<DT>(wf, vf[nb][ks], acc[nb]);
            }
            if (PASS == 1) {
#pragma unroll
                for (int nb = 0; nb < Geo::NB; ++nb) {
                    // key of accumulator 0 minus the last key this row sees (S < 2^31: the difference fits)
                    const int32_t rel = (int32_t)(s0 + sub * 32 + 4 * kg - diag - (wown0 + nb * 32 + n));
                    float x[16], mx = KVP_NEG_INF;
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        x[i] = acc[nb][i];
                        if (MASK && rel + (i & 3) + 8 * (i >> 2) > 0) x[i] = KVP_NEG_INF;   // the accumulator's key lies above the diagonal
                        mx = fmaxf(mx, x[i]);
                    }
                    const float mn = fmaxf(m[nb], mx);
                    const float off = mn == KVP_NEG_INF ? 0.f : -mn * a.c;
                    float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int i = 0; i < 16; ++i) s[i >> 2] += __builtin_amdgcn_exp2f(fmaf(x[i], a.c, off));
                    z[nb] = z[nb] * __builtin_amdgcn_exp2f(fmaf(m[nb], a.c, off)) + ((s[0] + s[1]) + (s[2] + s[3]));
                    m[nb] = mn;
                }
            } else {
                const float* lt = lsep + s0 + sub * 32 + 4 * kg;
                const float* rt = rspp + s0 + sub * 32 + 4 * kg;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 l4 = *reinterpret_cast<const float4*>(lt + 8 * q), r4 = *reinterpret_cast<const float4*>(rt + 8 * q);
                    const float l[4] = {l4.x, l4.y, l4.z, l4.w}, r[4] = {r4.x, r4.y, r4.z, r4.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int nb = 0; nb < Geo::NB; ++nb)
                            m[nb] = fmaxf(m[nb], __builtin_amdgcn_exp2f(fmaf(acc[nb][4 * q + e], a.c, -l[e])) * r[e]);
                }
            }
        }
    };
    uint32_t bufc = 0, bufn = Geo::TILEB;
    dma_wait<0>();   // this wave's part of the first tile has landed
    __syncthreads();
    for (int64_t t = t_first; t < t_last; ++t) {
        if (t + 1 < t_last) request_tile(t + 1, bufn);   // into the buffer tile t - 1 left at the last barrier
        const int64_t s0 = t * Geo::WT;
        // (workgroup-uniform) does the tile reach past the keys the FIRST owned row of the workgroup sees?
        if (PASS == 1 && s0 + Geo::WT - 1 - diag > own0) tile_body(std::true_type{}, s0, bufc);
        else tile_body(std::false_type{}, s0, bufc);
        dma_wait<0>();   // tile t + 1 has landed (this wave's part; the barrier covers the others)
        __syncthreads();
        const uint32_t tmp = bufc; bufc = bufn; bufn = tmp;
    }
#pragma unroll
    for (int nb = 0; nb < Geo::NB; ++nb) {
        const int64_t s = wown0 + nb * 32 + n;
        if (PASS == 1) {   // the two lane halves hold the two halves of every 32 keys
            float m2 = m[nb] * a.c, z2 = z[nb];
            wave_softmax_merge<32, 32>(m2, z2);
            if (kg == 0 && s < a.Lq) {
                a.pm[(int64_t)split * a.nrow + bh * a.Lq + s] = m2;
                a.pz[(int64_t)split * a.nrow + bh * a.Lq + s] = z2;
            }
        } else {
            const float v = fmaxf(m[nb], __shfl_xor(m[nb], 32));
            if (kg == 0 && s < a.ctx) a.part[(int64_t)split * a.npart + (int64_t)row * a.ctx + s] = v * (a.cs ? a.cs[bh * a.ctx + s] : 1.f);
        }
    }
}

// ---- generic path: any D, any dtype, any alignment (float32 modules, the tiny test models: D = 6).  Correctness only. ------------------------
// pass 1: a wave per query row, lane l takes the keys l, l + 64, .. of V(t); one partial per row (nks = 1)
template <int DT>
__global__ __launch_bounds__(KZ_THREADS) void kvzip_p1_generic(KzArgs a) {
    using T = typename Elem<DT>::T;
    const int64_t r = (int64_t)blockIdx.x * (KZ_THREADS / 64) + (threadIdx.x >> 6);   // (b * Hq + hq) * Lq + t
    const int lane = threadIdx.x & 63;
    if (r >= a.nrow) return;
    const int64_t t = r % a.Lq, bh = r / a.Lq;
    const int64_t b = bh / a.Hq, hkv = (bh % a.Hq) / a.G;
    const T* qr = (const T*)a.qrot + r * a.D;
    const T* kb = (const T*)a.k + b * a.k_sb + hkv * a.k_sh;
    const int64_t nvis = a.sink + a.ctx + t + 1;
    float m = KVP_NEG_INF, z = 0.f;
    for (int64_t v = lane; v < nvis; v += 64) {
        const T* kr = kb + kz_key_row(a, v) * a.k_ss;
        float dot = 0.f;
        for (int d = 0; d < a.D; ++d) dot = fmaf(Elem<DT>::ld(qr + d), Elem<DT>::ld(kr + d), dot);
        softmax_merge(m, z, dot * a.c, 1.f);
    }
    wave_softmax_merge(m, z);
    if (lane == 0) { a.pm[r] = m; a.pz[r] = z; }
}
// pass 2: a wave per (b, kv head, chunk key), lane l takes the rows l, l + 64, .. of the G * Lq rows of the group
template <int DT>
__global__ __launch_bounds__(KZ_THREADS) void kvzip_p2_generic(KzArgs a) {
    using T = typename Elem<DT>::T;
    const int64_t u = (int64_t)blockIdx.x * (KZ_THREADS / 64) + (threadIdx.x >> 6);   // (b * Hkv + h) * ctx + j
    const int lane = threadIdx.x & 63;
    if (u >= a.npart) return;
    const int64_t j = u % a.ctx, row = u / a.ctx;
    const int64_t b = row / a.Hkv, h = row % a.Hkv;
    const T* kr = (const T*)a.k + b * a.k_sb + h * a.k_sh + (a.start + j) * a.k_ss;
    float mx = 0.f;
    for (int64_t i = lane; i < a.G * a.Lq; i += 64) {
        const int64_t t = i % a.Lq, bh = b * a.Hq + h * a.G + i / a.Lq;
        const T* qr = (const T*)a.qrot + (bh * a.Lq + t) * a.D;
        float dot = 0.f;
        for (int d = 0; d < a.D; ++d) dot = fmaf(Elem<DT>::ld(qr + d), Elem<DT>::ld(kr + d), dot);
        mx = fmaxf(mx, exp2f(fmaf(dot, a.c, -a.lse[bh * a.Lqp + t])) * a.rsp[b * a.Lqp + t] * (a.cs ? a.cs[bh * a.ctx + j] : 1.f));
    }
    mx = wave_max(mx);
    if (lane == 0) a.out[row * a.out_stride + j] = mx;
}

// ---- lse[bh, t] = M + log2(Z) over the nks partials, in split order; the padding of lse (+inf) and of the row scales (0) ---------------------
__global__ __launch_bounds__(KZ_THREADS) void kz_combine_kernel(KzArgs a, int64_t BHq) {
    const int64_t i = (int64_t)blockIdx.x * KZ_THREADS + threadIdx.x;
    if (i >= BHq * a.Lqp) return;
    const int64_t t = i % a.Lqp, bh = i / a.Lqp;
    float lse = __builtin_huge_valf();
    if (t < a.Lq) {
        float m = KVP_NEG_INF, z = 0.f;
        for (uint32_t ks = 0; ks < a.nks; ++ks) softmax_merge(m, z, a.pm[(int64_t)ks * a.nrow + bh * a.Lq + t], a.pz[(int64_t)ks * a.nrow + bh * a.Lq + t]);
        lse = m + log2f(z);
    }
    a.lse[i] = lse;
    if (bh % a.Hq == 0) {
        const int64_t b = bh / a.Hq;
        a.rsp[b * a.Lqp + t] = t < a.Lq ? (a.rs ? a.rs[b * a.Lq + t] : 1.f) : 0.f;
    }
}

// ---- out[row, j] = max over the nsplit partial maxima ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(KZ_THREADS) void kz_merge_kernel(KzArgs a, uint32_t nsplit) {
    const int64_t i = (int64_t)blockIdx.x * KZ_THREADS + threadIdx.x;
    if (i >= a.npart) return;
    float mx = a.part[i];
    for (uint32_t s = 1; s < nsplit; ++s) mx = fmaxf(mx, a.part[(int64_t)s * a.npart + i]);
    a.out[(i / a.ctx) * a.out_stride + i % a.ctx] = mx;
}

// ---- host: the split of both passes and the workspace layout, from the shape alone ----------------------------------------------------------
struct KzPlan {
    bool mfma_shape;              // dtype and D of the matrix-core path (the alignment of the rows is the call's to test)
    int64_t Lqp;
    uint32_t nks, tps, ntt, nkt, nrs, rps;
};

KzPlan kz_plan(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Lq, int64_t D, int64_t sink, int64_t ctx) {
    KzPlan p{};
    p.mfma_shape = dtype != KVP_F32 && (D == 64 || D == 96 || D == 128 || D == 256);
    p.Lqp = (Lq + KZ_PAD - 1) / KZ_PAD * KZ_PAD;
    p.nks = 1;
    if (!p.mfma_shape) return p;
    const int64_t WT = D == 256 ? KzGeo<256>::WT : KzGeo<128>::WT, TOK = D == 256 ? KzGeo<256>::TOK : KzGeo<128>::TOK;
    p.ntt = (uint32_t)((Lq + TOK - 1) / TOK);
    const int64_t ntile = (sink + ctx + Lq + WT - 1) / WT;
    const int64_t nks = std::min(ntile, std::max<int64_t>(1, KZ_UNITS / (B * Hq * p.ntt)));
    p.tps = (uint32_t)((ntile + nks - 1) / nks);
    p.nks = (uint32_t)((ntile + p.tps - 1) / p.tps);
    p.nkt = (uint32_t)((ctx + TOK - 1) / TOK);
    const int64_t rt = (Lq + WT - 1) / WT;
    const int64_t nrs = std::min(rt, std::max<int64_t>(1, KZ_UNITS / (B * Hq * p.nkt)));
    const int64_t tpr = (rt + nrs - 1) / nrs;
    p.nrs = (uint32_t)((rt + tpr - 1) / tpr);
    p.rps = (uint32_t)(tpr * WT);
    return p;
}

struct KzWs {
    void* qrot;
    float *pm, *pz, *lse, *rsp, *part;
    size_t bytes;
};
KzWs kz_carve(void* ws, const KzPlan& p, int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Lq, int64_t D, int64_t ctx) {
    KvpArena ar(ws);
    KzWs w;
    w.qrot = ar.take<char>((size_t)(B * Hq * Lq * D) * kvp_elem_size(dtype));
    w.pm = ar.take<float>((size_t)p.nks * B * Hq * Lq);
    w.pz = ar.take<float>((size_t)p.nks * B * Hq * Lq);
    w.lse = ar.take<float>((size_t)(B * Hq * p.Lqp));
    w.rsp = ar.take<float>((size_t)(B * p.Lqp));
    w.part = ar.take<float>(p.mfma_shape ? (size_t)(Hq / Hkv) * p.nrs * B * Hkv * ctx : 0);
    w.bytes = ar.bytes();
    return w;
}

template <int DT, int D>
void kz_mfma_launch(const KzArgs& a, int64_t B, hipStream_t st) {
    KVP_LAUNCH("kvzip_p1_mfma", st, kvzip_mfma_kernel<DT, D, 1><<<(uint32_t)(B * a.Hq * a.ntt * a.nks), KZ_THREADS, 0, st>>>(a));
    KVP_LAUNCH("kvzip_combine", st, kz_combine_kernel<<<(uint32_t)((B * a.Hq * a.Lqp + KZ_THREADS - 1) / KZ_THREADS), KZ_THREADS, 0, st>>>(a, B * a.Hq));
    KVP_LAUNCH("kvzip_p2_mfma", st, kvzip_mfma_kernel<DT, D, 2><<<(uint32_t)(B * a.Hq * a.nrs * a.nkt), KZ_THREADS, 0, st>>>(a));
    KVP_LAUNCH("kvzip_merge", st, kz_merge_kernel<<<(uint32_t)((a.npart + KZ_THREADS - 1) / KZ_THREADS), KZ_THREADS, 0, st>>>(a, a.G * a.nrs));
}
template <int DT>
void kz_mfma_run(const KzArgs& a, int64_t B, hipStream_t st) {
    if (a.D == 64) kz_mfma_launch<DT, 64>(a, B, st);
    else if (a.D == 96) kz_mfma_launch<DT, 96>(a, B, st);
    else if (a.D == 128) kz_mfma_launch<DT, 128>(a, B, st);
    else kz_mfma_launch<DT, 256>(a, B, st);
}

}  // namespace

// ================================================================================================================================
extern "C" size_t kvp_kvzip_score_workspace_bytes(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Lq, int64_t D, int64_t sink,
                                                  int64_t ctx) {
    if (B < 1 || Hkv < 1 || Hq < 1 || Hq % Hkv != 0 || Lq < 1 || D < 1 || sink < 0 || ctx < 1) return 0;
    return kz_carve(nullptr, kz_plan(dtype, B, Hq, Hkv, Lq, D, sink, ctx), dtype, B, Hq, Hkv, Lq, D, ctx).bytes;
}

extern "C" int kvp_kvzip_score(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_ss, const void* cos, const void* sin, int64_t cs_sb,
                               int64_t cs_sw, const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss, int dtype, int64_t B, int64_t Hq,
                               int64_t Hkv, int64_t S, int64_t Lq, int64_t D, int64_t sink, int64_t start, int64_t end,
                               const float* row_scale, const float* col_scale, float* out, int64_t out_stride, void* ws, size_t ws_bytes,
                               kvp_stream_t stream) {
    KVP_CHECK_DTYPE("kvp_kvzip_score", dtype);
    KVP_CHECK_ARG(Hkv >= 1 && Hq >= 1 && Hq % Hkv == 0, "kvp_kvzip_score: Hq %% Hkv != 0 (%lld, %lld)", (long long)Hq, (long long)Hkv);
    KVP_CHECK_ARG(B >= 1 && Lq >= 1 && D >= 2 && D % 2 == 0 && S > Lq && S < ((int64_t)1 << 31), "kvp_kvzip_score: bad shape B=%lld S=%lld Lq=%lld D=%lld",
                  (long long)B, (long long)S, (long long)Lq, (long long)D);
    KVP_CHECK_ARG(0 <= sink && sink <= start && start < end && end <= S - Lq, "kvp_kvzip_score: need 0 <= sink <= start < end <= S - Lq (%lld, %lld, %lld, %lld)",
                  (long long)sink, (long long)start, (long long)end, (long long)(S - Lq));
    const int64_t ctx = end - start;
    KVP_CHECK_ARG(out_stride >= ctx || B * Hkv == 1, "kvp_kvzip_score: out_stride %lld < end - start", (long long)out_stride);
    KVP_CHECK_ARG(q && cos && sin && k && out, "kvp_kvzip_score: null pointer");
    const KzPlan p = kz_plan(dtype, B, Hq, Hkv, Lq, D, sink, ctx);
    KVP_CHECK_ARG(B * Hq * (int64_t)std::max(p.ntt * p.nks, p.nrs * p.nkt) < ((int64_t)1 << 31) && B * Hq * p.Lqp < ((int64_t)1 << 40),
                  "kvp_kvzip_score: too many rows (B * Hq * Lq)");
    const KzWs w = kz_carve(ws, p, dtype, B, Hq, Hkv, Lq, D, ctx);
    if (int rc = kvp_check_workspace("kvp_kvzip_score", ws, ws_bytes, w.bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;

    const int64_t half_elems = B * Hq * Lq * (D / 2);
    const uint32_t rope_blocks = (uint32_t)std::min<int64_t>((half_elems + KZ_THREADS - 1) / KZ_THREADS, 1 << 20);
    KVP_DISPATCH_DTYPE(dtype, {
        using T = typename Elem<DT>::T;
        KVP_LAUNCH("kvzip_rope", st, kz_rope_kernel<DT><<<rope_blocks, KZ_THREADS, 0, st>>>((const T*)q, q_sb, q_sh, q_ss, (const T*)cos, (const T*)sin,
                                                                                            cs_sb, cs_sw, B, Hq, Lq, D, (T*)w.qrot));
    });

    KzArgs a;
    a.qrot = w.qrot; a.k = k;
    a.k_sb = k_sb; a.k_sh = k_sh; a.k_ss = k_ss;
    a.Hq = (int)Hq; a.Hkv = (int)Hkv; a.G = (int)(Hq / Hkv); a.D = (int)D;
    a.S = S; a.Lq = Lq; a.Lqp = p.Lqp; a.sink = sink; a.start = start; a.ctx = ctx;
    a.c = (float)(1.4426950408889634 / sqrt((double)D));
    a.pm = w.pm; a.pz = w.pz; a.lse = w.lse; a.rsp = w.rsp;
    a.rs = row_scale; a.cs = col_scale;
    a.part = w.part; a.out = out; a.out_stride = out_stride;
    a.nrow = B * Hq * Lq; a.npart = B * Hkv * ctx;
    a.nks = p.nks; a.tps = p.tps; a.ntt = p.ntt; a.nkt = p.nkt; a.nrs = p.nrs; a.rps = p.rps;

    const KvpRows keys{k, k_sb, k_sh, k_ss};
    if (p.mfma_shape && keys.aligned(16, 2)) {
        if (dtype == KVP_F16) kz_mfma_run<KVP_F16>(a, B, st);
        else kz_mfma_run<KVP_BF16>(a, B, st);
    } else {
        a.nks = 1;
        const uint32_t g1 = (uint32_t)((a.nrow + KZ_THREADS / 64 - 1) / (KZ_THREADS / 64)), g2 = (uint32_t)((a.npart + KZ_THREADS / 64 - 1) / (KZ_THREADS / 64));
        KVP_DISPATCH_DTYPE(dtype, {
            KVP_LAUNCH("kvzip_p1_generic", st, kvzip_p1_generic<DT><<<g1, KZ_THREADS, 0, st>>>(a));
            KVP_LAUNCH("kvzip_combine", st, kz_combine_kernel<<<(uint32_t)((B * Hq * a.Lqp + KZ_THREADS - 1) / KZ_THREADS), KZ_THREADS, 0, st>>>(a, B * Hq));
            KVP_LAUNCH("kvzip_p2_generic", st, kvzip_p2_generic<DT><<<g2, KZ_THREADS, 0, st>>>(a));
        });
    }
    KVP_CHECK_LAUNCH("kvp_kvzip_score");
    return KVP_OK;
}
