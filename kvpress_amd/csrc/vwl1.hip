// CriticalKV's rescale (kvpress/presses/criticalkv_press.py:57-76, :87, :174-175; include/kvpress_hip.h: kvp_vwl1norm_*): the L1 norm of
// every value row pushed through the output projection, averaged over the G query heads of its kv head,
//     norm[b,k,s] = (1/G) sum_g sum_c | sum_d v[b,k,s,d] * wo[c, (k G + g) D + d] |,      out = norm  or  (scores + eps) * norm.
// o_proj.weight is [hidden, Hq D] row-major: the column block of query head h is `hidden` rows of D contiguous elements, a key tile's
// layout, so "V tile times Wo rows, transposed" is a QK^T with an abs-sum where the softmax was.  Nothing of size [S, hidden] or [Hq, S]
// exists: a workgroup owns a tile of tokens of one (b, kv head), keeps their value rows in registers for the whole kernel (the MFMA's B
// operand: tokens on the column side, a lane owns one token) and streams the G column blocks of Wo through LDS, 128 rows a tile.
// kvp_scores_fill_prefix (:169-171, :177-179) is the per-head prefix scatter of the two-stage selection.  No atomics: bit-identical runs.
#include <math.h>

#include <type_traits>

#include "kvp_mfma.h"

namespace {

constexpr int VW_THREADS = 256;   // 4 waves
constexpr int VW_MAX_XCD = 8;

struct VwArgs {
    const void *v, *wo;
    int64_t v_sb, v_sh, v_ss, wo_ld;
    int Hkv, G;
    int64_t S, hidden;
    const float* sin;    // scores_in (null: out = norm)
    int64_t sin_stride;
    float eps;
    float* out;          // [B * Hkv, S]
    uint32_t ntok, nunit, per_xcd;   // token tiles per row, workgroups with work, units per XCD (matrix-core path)
};

// norm -> out: (scores + eps) * norm, the add and the product rounded separately, in that order (criticalkv_press.py:87)
__device__ __forceinline__ void vw_store(const VwArgs& a, int64_t row, int64_t s, float total) {
    const float norm = total / (float)a.G;
    a.out[row * a.S + s] = a.sin ? __fmul_rn(__fadd_rn(a.sin[row * a.sin_stride + s], a.eps), norm) : norm;
}

// ---- matrix-core path: bf16 / f16, D in {64, 96, 128, 256}, 16-byte aligned rows -------------------------------------------------------
// Geometry.  Wave w owns NB blocks of 32 tokens (256 tokens a workgroup for D <= 128, 128 for D = 256); their value rows are DK k-steps of
// uint4 per block, loaded once.  A Wo tile is 128 LDS rows of kvp_mfma.h's swizzled key tile, filled by LDS-DMA and double-buffered; D = 256
// puts the two 256-byte halves of a Wo row into two consecutive LDS rows (64 Wo rows a tile), so one geometry serves every D.  The tiles
// of the G heads follow each other as one sequence (tile t of G * nct: head t / nct, rows (t % nct) * WT ..).  acc = Wo_rows x V^T per 32 Wo rows:
// lane (n, half) holds rows {0..3, 8..11, 16..19, 24..27} + 4 * half of token n, their |x| are added with the source modifier -- four chains of
// four to a sub-tile's partial, the partials to the head's sum, the heads' to the total: short chains, no cross-lane work until the two
// lane halves meet at the end.  Rows past `hidden` are requested clamped to the last row (an LDS-DMA request that skipped them would
// leave stale LDS behind) and masked to exactly 0 in the one tail tile.
// Order of the workgroups.  Blocks are dealt round-robin over the XCDs, so block b works on unit (b % 8) * per_xcd + b / 8 of the
// row-major (row, token tile) list: the workgroups resident on one XCD share a (b, kv head) and walk the same G * hidden * D * 2 bytes
// of Wo (4 MiB for Llama-3.1-8B: the XCD's L2) at about the same position.
template <int D> struct VwGeo : KTileGeo<(D == 256 ? 8 : D / 16), VW_THREADS> {
    using Base = KTileGeo<(D == 256 ? 8 : D / 16), VW_THREADS>;
    static constexpr int DK = D / 16;                  // MFMA k-steps of a head
    static constexpr int HALVES = D == 256 ? 2 : 1;    // LDS rows per Wo row
    static constexpr int WT = Base::TILE / HALVES;     // Wo rows per tile
    static constexpr int SUBS = WT / 32;
    static constexpr int NB = D <= 128 ? 2 : 1;        // 32-token blocks per wave
    static constexpr int TOK = (VW_THREADS / 64) * 32 * NB;
};

template <int DT, int D>
__global__ __launch_bounds__(VW_THREADS, 2) void vwl1_mfma_kernel(VwArgs a) {
    using Geo = VwGeo<D>;
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * Geo::TILEB];
    const uint32_t unit = (blockIdx.x % VW_MAX_XCD) * a.per_xcd + blockIdx.x / VW_MAX_XCD;
    if (unit >= a.nunit) return;
    const uint32_t row = unit / a.ntok, tt = unit - row * a.ntok;   // row = b * Hkv + kv head
    const uint32_t b = row / a.Hkv, kh = row - b * a.Hkv;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t n = lane & 31, kg = lane >> 5;
    const int64_t tok0 = (int64_t)tt * Geo::TOK + wv * (32 * Geo::NB);

    // the value rows of this wave's tokens (B operand): k-step ks, lane half kg = elements 16 ks + 8 kg .. + 8; tokens past S are zero rows
    uint4 vf[Geo::NB][Geo::DK];
    const char* vb = static_cast<const char*>(a.v) + ((int64_t)b * a.v_sb + (int64_t)kh * a.v_sh) * 2;
#pragma unroll
    for (int nb = 0; nb < Geo::NB; ++nb) {
        const int64_t s = tok0 + nb * 32 + n;
        const char* vr = vb + s * a.v_ss * 2 + kg * 16;
#pragma unroll
        for (int ks = 0; ks < Geo::DK; ++ks) vf[nb][ks] = s < a.S ? *reinterpret_cast<const uint4*>(vr + ks * 32) : make_uint4(0, 0, 0, 0);
    }

    const uint32_t nct = (uint32_t)((a.hidden + Geo::WT - 1) / Geo::WT);   // column tiles of a head
    const uint32_t ntiles = nct * a.G;
    const char* wb = static_cast<const char*>(a.wo) + (int64_t)kh * a.G * D * 2;
    const int64_t wrow_bytes = a.wo_ld * 2;
    const uint32_t ldsbase = KVP_LDS_ADDR(lds);
    const uint32_t rrow = Geo::RPW * wv + lane / Geo::CPR;        // this lane's LDS row inside a request
    const uint32_t rchunk = (lane % Geo::CPR) ^ Geo::sw(rrow);    // (a request's first row is a multiple of the swizzle period)
    auto request_tile = [&](uint32_t t, uint32_t buf_off) {
        const uint32_t g = t / nct, c0 = (t - g * nct) * Geo::WT;
        const char* hb = wb + (int64_t)g * D * 2 + (rchunk << 4);
#pragma unroll
        for (int j = 0; j < Geo::NREQ; ++j) {
            const uint32_t lr = Geo::RPR * j + rrow;
            const int64_t c = min((int64_t)c0 + lr / Geo::HALVES, a.hidden - 1);   // rows past hidden: the last row (masked below)
            const char* gp = hb + c * wrow_bytes + (lr % Geo::HALVES) * 256;
            const uint32_t la = __builtin_amdgcn_readfirstlane(ldsbase + buf_off + (Geo::RPR * j + Geo::RPW * wv) * Geo::ROWB);
            if (Geo::NCH == Geo::CPR) lds_dma16(la, gp);
            else lds_dma16_if(rchunk < (uint32_t)Geo::NCH, la, gp);
        }
    };
    request_tile(0, 0);

    float total[Geo::NB], hsum[Geo::NB];
#pragma unroll
    for (int nb = 0; nb < Geo::NB; ++nb) total[nb] = hsum[nb] = 0.f;
    // one tile: per 32 Wo rows DK x NB MFMAs on fresh accumulators, then the |x| of a lane's 16 rows in four chains of four (TAIL: the rows
    // past hidden as exact zeros)
    auto tile_body = [&](auto tail_tag, int64_t c0, uint32_t buf) {
        constexpr bool TAIL = decltype(tail_tag)::value;
#pragma unroll
        for (int sub = 0; sub < Geo::SUBS; ++sub) {
            f32x16 acc[Geo::NB];
#pragma unroll
            for (int nb = 0; nb < Geo::NB; ++nb)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[nb][i] = 0.f;
#pragma unroll
            for (int ks = 0; ks < Geo::DK; ++ks) {
                const uint32_t ch = ks * 2 + kg;                                                       // 16-byte chunk of the Wo row
                const uint32_t lr = (sub * 32 + n) * Geo::HALVES + (Geo::HALVES == 2 ? ch >> 4 : 0);   // its LDS row
                const uint4 wf = *reinterpret_cast<const uint4*>(lds + buf + lr * Geo::ROWB + (((ch & (Geo::CPR - 1)) ^ Geo::sw(lr)) << 4));
#pragma unroll
                for (int nb = 0; nb < Geo::NB; ++nb) acc[nb] = mma32<DT>(wf, vf[nb][ks], acc[nb]);
            }
#pragma unroll
            for (int nb = 0; nb < Geo::NB; ++nb) {
                float p[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    float x = fabsf(acc[nb][i]);
                    if (TAIL && c0 + sub * 32 + (i & 3) + 8 * (i >> 2) + 4 * kg >= a.hidden) x = 0.f;   // the accumulator's Wo row
                    p[i >> 2] += x;
                }
                hsum[nb] += (p[0] + p[1]) + (p[2] + p[3]);
            }
        }
    };
    uint32_t bufc = 0, bufn = Geo::TILEB;
    dma_wait<0>();   // this wave's part of tile 0 has landed
    __syncthreads();
    uint32_t ct = 0;   // column tile of the head
    for (uint32_t t = 0; t < ntiles; ++t) {
        if (t + 1 < ntiles) request_tile(t + 1, bufn);   // into the buffer tile t - 1 left at the last barrier
        const int64_t c0 = (int64_t)ct * Geo::WT;
        const bool tail = c0 + Geo::WT > a.hidden;       // (workgroup-uniform)
        if (!tail) tile_body(std::false_type{}, c0, bufc);
        else tile_body(std::true_type{}, c0, bufc);
        if (++ct == nct) {   // the head is done
            ct = 0;
#pragma unroll
            for (int nb = 0; nb < Geo::NB; ++nb) {
                total[nb] += hsum[nb];
                hsum[nb] = 0.f;
            }
        }
        dma_wait<0>();   // tile t + 1 has landed (this wave's part; the barrier covers the others)
        __syncthreads();
        const uint32_t tmp = bufc; bufc = bufn; bufn = tmp;
    }
#pragma unroll
    for (int nb = 0; nb < Geo::NB; ++nb) {
        const float tot = total[nb] + __shfl_xor(total[nb], 32);   // the two lane halves hold the two halves of every 32 Wo rows
        const int64_t s = tok0 + nb * 32 + n;
        if (kg == 0 && s < a.S) vw_store(a, row, s, tot);
    }
}

// ---- generic path: any D, any dtype, any alignment (float32 modules, the tiny test models: D = 16).  Correctness only: a wave per token,
// lane l owns Wo rows l, l + 64, .. of every head; the heads' sums meet by a butterfly, head after head.
template <int DT>
__global__ __launch_bounds__(VW_THREADS) void vwl1_generic_kernel(VwArgs a, int D) {
    using T = typename Elem<DT>::T;
    const int64_t row = blockIdx.y;
    const int64_t b = row / a.Hkv, kh = row % a.Hkv;
    const int64_t s = (int64_t)blockIdx.x * (VW_THREADS / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (s >= a.S) return;
    const T* vr = (const T*)a.v + b * a.v_sb + kh * a.v_sh + s * a.v_ss;
    float total = 0.f;
    for (int g = 0; g < a.G; ++g) {
        const T* wh = (const T*)a.wo + (kh * a.G + g) * D;
        float hs = 0.f;
        for (int64_t c = lane; c < a.hidden; c += 64) {
            const T* wr = wh + c * a.wo_ld;
            float dot = 0.f;
            for (int d = 0; d < D; ++d) dot = fmaf(Elem<DT>::ld(vr + d), Elem<DT>::ld(wr + d), dot);
            hs += fabsf(dot);
        }
        total += wave_sum(hs);
    }
    if (lane == 0) vw_store(a, row, s, total);
}

// ---- kvp_scores_fill_prefix: scores[r, idx[r, j]] = value for j < counts[r] ---------------------------------------------------------------
__global__ __launch_bounds__(256) void fill_prefix_kernel(float* __restrict__ scores, int64_t row_stride, const int32_t* __restrict__ idx,
                                                          uint32_t n, uint32_t S, const int32_t* __restrict__ counts, float value) {
    float* row = scores + (int64_t)blockIdx.y * row_stride;
    const int32_t* ir = idx + (size_t)blockIdx.y * n;
    const uint32_t cnt = (uint32_t)max(0, min(counts[blockIdx.y], (int32_t)n));
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < cnt; j += gridDim.x * blockDim.x) {
        const int32_t p = ir[j];
        if (p >= 0 && (uint32_t)p < S) row[p] = value;
    }
}

bool vw_mfma_ok(int dtype, int64_t D, int64_t B, int64_t Hkv, int64_t S, const KvpRows& v, const void* wo, int64_t wo_ld) {
    if (dtype == KVP_F32) return false;
    if (D != 64 && D != 96 && D != 128 && D != 256) return false;
    const int64_t tok = D <= 128 ? VwGeo<128>::TOK : VwGeo<256>::TOK;
    if ((S + tok - 1) / tok * B * Hkv >= ((int64_t)1 << 31) - 8 * VW_MAX_XCD) return false;
    return v.aligned(16, 2) && (((uintptr_t)wo | (uintptr_t)wo_ld * 2) & 15) == 0;
}

template <int DT, int D>
void vw_mfma_launch(VwArgs& a, int64_t B, hipStream_t st) {
    a.ntok = (uint32_t)((a.S + VwGeo<D>::TOK - 1) / VwGeo<D>::TOK);
    a.nunit = (uint32_t)(a.ntok * B * a.Hkv);
    a.per_xcd = (a.nunit + VW_MAX_XCD - 1) / VW_MAX_XCD;
    KVP_LAUNCH("vwl1_mfma", st, vwl1_mfma_kernel<DT, D><<<a.per_xcd * VW_MAX_XCD, VW_THREADS, 0, st>>>(a));
}

template <int DT>
void vw_mfma_run(VwArgs& a, int64_t B, int64_t D, hipStream_t st) {
    if (D == 64) vw_mfma_launch<DT, 64>(a, B, st);
    else if (D == 96) vw_mfma_launch<DT, 96>(a, B, st);
    else if (D == 128) vw_mfma_launch<DT, 128>(a, B, st);
    else vw_mfma_launch<DT, 256>(a, B, st);
}

}  // namespace

// ================================================================================================================================
// Nothing of size [S, hidden] or [Hq, S] is ever stored: the entry needs no workspace (the query and the `ws` argument keep the shape of
// every other entry of the header).
extern "C" size_t kvp_vwl1norm_workspace_bytes(int64_t B, int64_t Hq, int64_t Hkv, int64_t S, int64_t D, int64_t hidden) {
    (void)B; (void)Hq; (void)Hkv; (void)S; (void)D; (void)hidden;
    return 0;
}

extern "C" int kvp_vwl1norm_rescale(const void* values, int64_t v_sb, int64_t v_sh, int64_t v_ss, int dtype, const void* wo, int64_t wo_ld,
                                    int64_t B, int64_t Hq, int64_t Hkv, int64_t S, int64_t D, int64_t hidden,
                                    const float* scores_in, int64_t scores_stride, float eps, float* out, void* ws, size_t ws_bytes,
                                    kvp_stream_t stream) {
    (void)ws; (void)ws_bytes;
    KVP_CHECK_DTYPE("kvp_vwl1norm_rescale", dtype);
    KVP_CHECK_ARG(Hkv >= 1 && Hq >= 1 && Hq % Hkv == 0, "kvp_vwl1norm_rescale: Hq %% Hkv != 0 (%lld, %lld)", (long long)Hq, (long long)Hkv);
    KVP_CHECK_ARG(hidden > 0, "kvp_vwl1norm_rescale: hidden must be positive (%lld)", (long long)hidden);
    KVP_CHECK_ARG(B >= 1 && S >= 1 && D >= 1 && (hidden == 1 || wo_ld >= Hq * D) && S < ((int64_t)1 << 31) && hidden < ((int64_t)1 << 31) &&
                      (!scores_in || scores_stride >= S || B * Hkv == 1),
                  "kvp_vwl1norm_rescale: bad shape");
    KVP_CHECK_ARG(values && wo && out, "kvp_vwl1norm_rescale: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const KvpRows v{values, v_sb, v_sh, v_ss};
    VwArgs a;
    a.v = values; a.wo = wo;
    a.v_sb = v_sb; a.v_sh = v_sh; a.v_ss = v_ss; a.wo_ld = wo_ld;
    a.Hkv = (int)Hkv; a.G = (int)(Hq / Hkv);
    a.S = S; a.hidden = hidden;
    a.sin = scores_in; a.sin_stride = scores_stride; a.eps = eps; a.out = out;
    a.ntok = a.nunit = a.per_xcd = 0;
    if (vw_mfma_ok(dtype, D, B, Hkv, S, v, wo, wo_ld)) {
        if (dtype == KVP_F16) vw_mfma_run<KVP_F16>(a, B, D, st);
        else vw_mfma_run<KVP_BF16>(a, B, D, st);
    } else {
        KVP_CHECK_ARG(B * Hkv <= 65535, "kvp_vwl1norm_rescale: more than 65535 rows (B * Hkv) on the generic kernel");
        const dim3 grid((unsigned)((S + VW_THREADS / 64 - 1) / (VW_THREADS / 64)), (unsigned)(B * Hkv));
        KVP_DISPATCH_DTYPE(dtype, KVP_LAUNCH("vwl1_generic", st, vwl1_generic_kernel<DT><<<grid, VW_THREADS, 0, st>>>(a, (int)D)));
    }
    KVP_CHECK_LAUNCH("kvp_vwl1norm_rescale");
    return KVP_OK;
}

extern "C" int kvp_scores_fill_prefix(float* scores, int64_t R, int64_t S, int64_t row_stride, const int32_t* idx, int64_t n,
                                      const int32_t* counts, float value, kvp_stream_t stream) {
    KVP_CHECK_ARG(R >= 0 && S >= 0 && n >= 0 && R <= 65535 && row_stride >= S && n < ((int64_t)1 << 31) && S < ((int64_t)1 << 31),
                  "kvp_scores_fill_prefix: bad shape R=%lld S=%lld n=%lld", (long long)R, (long long)S, (long long)n);
    if (R * n == 0) return KVP_OK;
    KVP_CHECK_ARG(scores && idx && counts, "kvp_scores_fill_prefix: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const uint32_t bx = (uint32_t)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 1024));
    KVP_LAUNCH("fill_prefix", st, fill_prefix_kernel<<<dim3(bx, (uint32_t)R), 256, 0, st>>>(scores, row_stride, idx, (uint32_t)n, (uint32_t)S, counts, value));
    KVP_CHECK_LAUNCH("kvp_scores_fill_prefix");
    return KVP_OK;
}
