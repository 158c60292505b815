// KVzap's surrogate scorer (kvpress/presses/kvzap_press.py:79-81 with the module bodies :33-35 / :38-45; include/kvpress_hip.h:
// kvp_kvzap_score) and DMSPress's threshold eviction (kvpress/presses/dms_press.py:106-112; kvp_threshold_count / kvp_threshold_select).
//     mlp:    out[b,o,s] = b2[o] + sum_j W2[o,j] * gelu(b1[j] + sum_k x[b,s,k] * W1[j,k])        (erf GELU, everything after the products float32)
//     linear: out[b,o,s] = b1[o] + sum_k x[b,s,k] * W1[o,k]                                      (N = 0)
// Nothing of extent S x N is stored: a workgroup of the matrix-core kernel owns a tile of tokens and ALL N hidden columns of it, so the
// bias, the GELU and layer two run on its accumulators.  No atomics anywhere: every sum has one fixed order, runs are bit-identical.
//
// What bounds the matrix-core kernel (Llama-3.1-8B: K 4096, N 512, Hout 8; 128 tokens a workgroup, 8 waves, one workgroup a CU because
// of its 160 KiB of LDS).  Every workgroup re-reads W1 from the L2s: 4 MiB + 1 MiB of x per 128 tokens, 5.1 GiB at 128k tokens, which at
// the ~10 TB/s qproj.hip measured for the L2 -> CU path is 0.55 ms of the 0.61 ms a call takes -- that stream is the
// bound, not the matrix cores (551 GFLOP: 0.22 ms at the bf16 peak; the call reaches 0.36 of it) and not the LDS (per k-step of 16 a wave
// reads 2 token and 4 weight fragments, 6 KiB, for 8 MFMAs 32x32x16: 96 of the 128 B/clk a CU's LDS gives).  A larger token tile would
// lift it; 128 accumulator registers a lane at two waves a SIMD are what forbids one.  The epilogue (128 erf a lane, no MFMA beside it:
// the CU's one workgroup is in it as a whole) is on top.  Non-temporal requests for the token rows were 5 % slower.
#include <math.h>

#include "kvp_mfma.h"

namespace {

struct ZapArgs {
    const void *x, *w1, *b1, *w2, *b2;
    int64_t x_sb, x_ss;          // element strides of the hidden states [B, S, K]
    uint32_t S, R;               // R = B * S tokens (token t: b = t / S, s = t % S)
    int K, N, Hout;              // N = 0: the linear model (w1 [Hout, K], b1 [Hout])
    float* out;                  // [B, Hout, S] through element strides
    int64_t o_sb, o_sh, o_ss;
    float* part;                 // few-rows path: [slices, R, Hout]
    uint32_t nslice;
};

__device__ __forceinline__ float zap_gelu(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f)); }

__device__ __forceinline__ float* zap_out(const ZapArgs& a, uint32_t t, uint32_t o) {
    const uint32_t b = t / a.S, s = t - b * a.S;
    return a.out + (int64_t)b * a.o_sb + (int64_t)o * a.o_sh + (int64_t)s * a.o_ss;
}
template <int DT> __device__ __forceinline__ const typename Elem<DT>::T* zap_row(const ZapArgs& a, uint32_t t) {
    const uint32_t b = t / a.S, s = t - b * a.S;
    return static_cast<const typename Elem<DT>::T*>(a.x) + (int64_t)b * a.x_sb + (int64_t)s * a.x_ss;
}
// the dot product of the 8 + 8 elements of two 16-byte vectors onto acc: one fma chain in element order
template <int DT> __device__ __forceinline__ float zap_dot8(const uint4& u, const float* wf, float acc) {
    float xf[8];
    unpack16<DT>(u, xf);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc = fmaf(xf[i], wf[i], acc);
    return acc;
}

// ---- matrix-core path: bf16 / f16, 16-byte aligned rows, K % 32 == 0, N % 32 == 0, 32 <= N <= 1024, Hout <= 16 -----------------------
// Geometry.  8 waves: wave w owns the token group tg = w & 1 (TSUB blocks of 32 tokens) and the column group cg = w >> 1 (the 32-column
// blocks cb = cg + 4 j, j < NBW, of the hidden layer); acc[ts][j] = W1 block x X block^T, so lane (n, half) holds hidden units
// 32 cb + {0..3, 8..11, 16..19, 24..27} + 4 half of token n.  N <= 512: TSUB 2, NBW 4, K tiles of 64 (128 tokens); N <= 1024: TSUB 1,
// NBW 8, K tiles of 32 (64 tokens) -- 128 accumulator registers either way.  An LDS tile is N weight rows followed by TOK token rows of
// KT elements, XOR-swizzled on the global side of the LDS-DMA (kvp_mfma.h), double-buffered.  Token rows past R are requested clamped
// to the last token (never stored); the K tail (K % 64 == 32) requests the chunks that exist and runs the k-steps that exist.
// Epilogue, in the LDS the tiles leave behind: W2 and b1 as float32; gelu in place; per output o one fma chain over the lane's hidden
// units in register order; the 8 partials (column group, lane half) of a token meet in LDS and are added in that order, then b2.
template <int TSUB_, int NBW_, int KT_> struct ZapGeo {
    static constexpr int THREADS = 512, WAVES = 8, CW = 4, TG = 2;
    static constexpr int TSUB = TSUB_, NBW = NBW_, KT = KT_;
    static constexpr int TOK = TG * TSUB * 32;
    static constexpr int NMAX = CW * NBW * 32;
    static constexpr int ROWB = KT * 2, CPR = ROWB / 16, RPW = 1024 / ROWB, KSTEPS = KT / 16;
    static constexpr int MAXG = ((NMAX + TOK) / RPW + WAVES - 1) / WAVES;   // row groups (one request each) a wave owns at most
    static __host__ __device__ __forceinline__ uint32_t sw(uint32_t row) { return CPR == 8 ? ((row >> 1) & 7u) : ((row >> 2) & 3u); }
    static size_t lds_bytes(int N, int Hout) {
        const size_t tiles = 2 * (size_t)(N + TOK) * ROWB, epi = ((size_t)Hout * N + N + (size_t)CW * 2 * Hout * TOK) * 4;
        return std::max(tiles, epi);
    }
};

template <int DT, class Geo>
__global__ __launch_bounds__(Geo::THREADS) void kvzap_mfma_kernel(ZapArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char zlds[];
    constexpr int TSUB = Geo::TSUB, NBW = Geo::NBW;
    const uint32_t lane = threadIdx.x & 63, wv = uni((uint32_t)(threadIdx.x >> 6));
    const uint32_t n = lane & 31, kg = lane >> 5;
    const uint32_t tg = wv & 1, cg = wv >> 1;
    const uint32_t N = (uint32_t)a.N, K = (uint32_t)a.K, NCB = N / 32;
    const uint32_t tok0 = blockIdx.x * Geo::TOK;
    const uint32_t rows = N + Geo::TOK, ngroups = rows / Geo::RPW, tileb = rows * Geo::ROWB;

    // this lane's part of the wave's requests: row group g = wv + 8 i, LDS row g RPW + lane / CPR, slot lane % CPR holding chunk slot ^ sw(row)
    const char* gptr[Geo::MAXG];
    const uint32_t rl = lane / Geo::CPR, slot = lane % Geo::CPR;
    uint32_t chunk_of[Geo::MAXG];
#pragma unroll
    for (int i = 0; i < Geo::MAXG; ++i) {
        const uint32_t row = min((wv + 8 * i) * Geo::RPW + rl, rows - 1);
        const uint32_t chunk = slot ^ Geo::sw(row);
        chunk_of[i] = chunk;
        if (row < N) {
            gptr[i] = static_cast<const char*>(a.w1) + ((int64_t)row * K) * 2 + chunk * 16;
        } else {
            const uint32_t t = min(tok0 + (row - N), a.R - 1);   // token rows past R: the last token (never stored)
            gptr[i] = reinterpret_cast<const char*>(zap_row<DT>(a, t)) + chunk * 16;
        }
    }
    const uint32_t ldsbase = KVP_LDS_ADDR(zlds);
    auto request_tile = [&](uint32_t kt, uint32_t buf_off) {
        const uint32_t k0 = kt * Geo::KT;
        const uint32_t nvc = min((uint32_t)Geo::CPR, (K - k0) / 8);   // 16-byte chunks of the row that exist in this tile
#pragma unroll
        for (int i = 0; i < Geo::MAXG; ++i) {
            const uint32_t g = wv + 8 * i;
            const uint32_t la = __builtin_amdgcn_readfirstlane(ldsbase + buf_off + min(g, ngroups - 1) * (Geo::RPW * Geo::ROWB));
            lds_dma16_if(g < ngroups && chunk_of[i] < nvc, la, gptr[i] + (int64_t)k0 * 2);   // (non-temporal requests for the token rows: 5 % slower)
        }
    };

    f32x16 acc[TSUB][NBW];
#pragma unroll
    for (int ts = 0; ts < TSUB; ++ts)
#pragma unroll
        for (int j = 0; j < NBW; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[ts][j][i] = 0.f;

    const uint32_t nkt = (K + Geo::KT - 1) / Geo::KT;
    request_tile(0, 0);
    uint32_t bufc = 0, bufn = tileb;
    dma_wait<0>();
    __syncthreads();
    for (uint32_t kt = 0; kt < nkt; ++kt) {
        if (kt + 1 < nkt) request_tile(kt + 1, bufn);   // into the buffer tile kt - 1 left at the last barrier
        const uint32_t ksteps = min((uint32_t)Geo::KSTEPS, (K - kt * Geo::KT) / 16);
#pragma unroll
        for (int ks = 0; ks < Geo::KSTEPS; ++ks) {
            if ((uint32_t)ks < ksteps) {   // (workgroup-uniform)
                const uint32_t ch = ks * 2 + kg;
                uint4 xf[TSUB];
#pragma unroll
                for (int ts = 0; ts < TSUB; ++ts) {
                    const uint32_t row = N + (tg * TSUB + ts) * 32 + n;
                    xf[ts] = *reinterpret_cast<const uint4*>(zlds + bufc + row * Geo::ROWB + ((ch ^ Geo::sw(row)) << 4));
                }
#pragma unroll
                for (int j = 0; j < NBW; ++j) {
                    const uint32_t cb = cg + Geo::CW * j;
                    if (cb < NCB) {        // (wave-uniform)
                        const uint32_t row = cb * 32 + n;
                        const uint4 wf = *reinterpret_cast<const uint4*>(zlds + bufc + row * Geo::ROWB + ((ch ^ Geo::sw(row)) << 4));
#pragma unroll
                        for (int ts = 0; ts < TSUB; ++ts) acc[ts][j] = mma32<DT>(wf, xf[ts], acc[ts][j]);
                    }
                }
            }
        }
        dma_wait<0>();   // tile kt + 1 has landed (this wave's part; the barrier covers the others)
        __syncthreads();
        const uint32_t tmp = bufc; bufc = bufn; bufn = tmp;
    }

    // ---- epilogue: every wave is past the last barrier, the tiles are dead ----
    using T = typename Elem<DT>::T;
    const uint32_t Hout = (uint32_t)a.Hout;
    float* w2s = reinterpret_cast<float*>(zlds);       // [Hout, N]
    float* b1s = w2s + Hout * N;                        // [N]
    float* red = b1s + N;                               // [CW * 2, Hout, TOK]
    for (uint32_t i = threadIdx.x; i < Hout * N; i += Geo::THREADS) w2s[i] = Elem<DT>::ld(static_cast<const T*>(a.w2) + i);
    for (uint32_t i = threadIdx.x; i < N; i += Geo::THREADS) b1s[i] = Elem<DT>::ld(static_cast<const T*>(a.b1) + i);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NBW; ++j) {
        const uint32_t cb = cg + Geo::CW * j;
        if (cb < NCB) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 bb = *reinterpret_cast<const float4*>(b1s + cb * 32 + 8 * q + 4 * kg);
                const float bq[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
                for (int ts = 0; ts < TSUB; ++ts)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[ts][j][4 * q + e] = zap_gelu(acc[ts][j][4 * q + e] + bq[e]);
            }
        }
    }
    for (uint32_t o = 0; o < Hout; ++o) {
        float p[TSUB];
#pragma unroll
        for (int ts = 0; ts < TSUB; ++ts) p[ts] = 0.f;
#pragma unroll
        for (int j = 0; j < NBW; ++j) {
            const uint32_t cb = cg + Geo::CW * j;
            if (cb < NCB) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 ww = *reinterpret_cast<const float4*>(w2s + o * N + cb * 32 + 8 * q + 4 * kg);
                    const float wq[4] = {ww.x, ww.y, ww.z, ww.w};
#pragma unroll
                    for (int ts = 0; ts < TSUB; ++ts)
#pragma unroll
                        for (int e = 0; e < 4; ++e) p[ts] = fmaf(wq[e], acc[ts][j][4 * q + e], p[ts]);
                }
            }
        }
#pragma unroll
        for (int ts = 0; ts < TSUB; ++ts) red[((cg * 2 + kg) * Hout + o) * Geo::TOK + (tg * TSUB + ts) * 32 + n] = p[ts];
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < Hout * Geo::TOK; e += Geo::THREADS) {
        const uint32_t o = e / Geo::TOK, tl = e - o * Geo::TOK, t = tok0 + tl;
        if (t < a.R) {
            float sum = red[o * Geo::TOK + tl];
#pragma unroll
            for (int q = 1; q < Geo::CW * 2; ++q) sum += red[(q * Hout + o) * Geo::TOK + tl];
            *zap_out(a, t, o) = sum + Elem<DT>::ld(static_cast<const T*>(a.b2) + o);
        }
    }
}

// ---- few-rows path (a decoding step: R = B * S <= 16 tokens): bf16 / f16, 16-byte aligned rows, K % 32 == 0, Hout <= 16 ---------------
// One workgroup per token tile would pull all of W1 through one CU.  Here a wave owns one row of W1 (mlp: hidden column j, all of K; linear:
// output o, a K slice of 512) and every token: the row's chunks are read once, the R dot products are fma chains in chunk order and meet
// by a butterfly.  mlp: the four waves of a workgroup put gelu(.) into LDS and thread (r, o) adds their W2[o, j] * h_j in wave order --
// one float32 partial of every output per slice of four columns.  A second launch adds the slices in slice order and the bias.
constexpr int ZR_THREADS = 256, ZR_MAXR = 16, ZR_KSLICE = 512;

template <int DT, bool MLP>
__global__ __launch_bounds__(ZR_THREADS) void kvzap_rows_kernel(ZapArgs a, uint32_t kslices) {
    using T = typename Elem<DT>::T;
    __shared__ float hs[ZR_THREADS / 64][ZR_MAXR];
    const uint32_t lane = threadIdx.x & 63, wv = uni((uint32_t)(threadIdx.x >> 6));
    const uint32_t grp = blockIdx.x / kslices, ksl = blockIdx.x - grp * kslices;
    const uint32_t j = grp * (ZR_THREADS / 64) + wv;                  // row of W1
    const uint32_t nrow = MLP ? (uint32_t)a.N : (uint32_t)a.Hout;
    const uint32_t kbeg = MLP ? 0u : ksl * ZR_KSLICE, kend = MLP ? (uint32_t)a.K : min((uint32_t)a.K, kbeg + ZR_KSLICE);
    float acc[ZR_MAXR];
#pragma unroll
    for (int r = 0; r < ZR_MAXR; ++r) acc[r] = 0.f;
    if (j < nrow) {
        const T* wr = static_cast<const T*>(a.w1) + (int64_t)j * a.K;
        for (uint32_t k = kbeg + lane * 8; k < kend; k += 64 * 8) {
            float wf[8];
            unpack16<DT>(*reinterpret_cast<const uint4*>(wr + k), wf);
#pragma unroll
            for (int r = 0; r < ZR_MAXR; ++r)
                if ((uint32_t)r < a.R) acc[r] = zap_dot8<DT>(*reinterpret_cast<const uint4*>(zap_row<DT>(a, r) + k), wf, acc[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < ZR_MAXR; ++r)
        if ((uint32_t)r < a.R) acc[r] = wave_sum(acc[r]);
    if (MLP) {
        const float bj = j < nrow ? Elem<DT>::ld(static_cast<const T*>(a.b1) + j) : 0.f;
#pragma unroll
        for (int r = 0; r < ZR_MAXR; ++r)
            if ((uint32_t)r < a.R && lane == 0) hs[wv][r] = j < nrow ? zap_gelu(acc[r] + bj) : 0.f;
        __syncthreads();
        const uint32_t e = threadIdx.x;
        if (e < a.R * (uint32_t)a.Hout) {
            const uint32_t r = e / a.Hout, o = e - r * a.Hout;
            float p = 0.f;
#pragma unroll
            for (int w = 0; w < ZR_THREADS / 64; ++w) {
                const uint32_t jw = grp * (ZR_THREADS / 64) + w;
                if (jw < nrow) p = fmaf(Elem<DT>::ld(static_cast<const T*>(a.w2) + (int64_t)o * a.N + jw), hs[w][r], p);
            }
            a.part[((size_t)blockIdx.x * a.R + r) * a.Hout + o] = p;
        }
    } else if (j < nrow && lane == 0) {
#pragma unroll
        for (int r = 0; r < ZR_MAXR; ++r)
            if ((uint32_t)r < a.R) a.part[((size_t)blockIdx.x * a.R + r) * a.Hout + j] = acc[r];
    }
}

// out[r, o] = bias[o] + the slices' partials in slice order.  linear: slice (grp, ksl) holds outputs 4 grp .. 4 grp + 3 only
template <int DT, bool MLP>
__global__ __launch_bounds__(256) void kvzap_rows_finish_kernel(ZapArgs a, uint32_t kslices) {
    using T = typename Elem<DT>::T;
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.R * (uint32_t)a.Hout) return;
    const uint32_t r = e / a.Hout, o = e - r * a.Hout;
    const uint32_t first = MLP ? 0u : (o / (ZR_THREADS / 64)) * kslices, count = MLP ? a.nslice : kslices;
    float sum = 0.f;
    for (uint32_t s = 0; s < count; ++s) sum += a.part[((size_t)(first + s) * a.R + r) * a.Hout + o];
    *zap_out(a, r, o) = sum + Elem<DT>::ld(static_cast<const T*>(MLP ? a.b2 : a.b1) + o);
}

// ---- the linear model over many tokens: bf16 / f16, aligned, K % 32 == 0, Hout <= 16.  Bound by reading x once.  mma16 with the rows of
// W1 as the A operand (output o < Hout; the other rows of the 16 are zeros) and 16 tokens as B, fragments straight from global memory: lane
// (n, kg) holds elements k + 8 kg .. + 8 of its row.  A workgroup owns 32 tokens and its four waves the k-steps w, w + 4, .. of them (a
// token's 256 consecutive bytes per round; 16 waves a CU keep the loads in flight that a stream needs); a fragment of W1 (64 KiB in all:
// L1 / L2) serves two token fragments.  The waves' partials meet in LDS and are added in wave order.  (A VALU form of this kernel was bound
// by its fmas at 3.3 TB/s; one wave per 64 tokens and all of K left half the chip idle at 32k tokens.)
constexpr int ZL_TB = 2, ZL_TOK = 16 * ZL_TB;   // 16-token blocks and tokens per workgroup
template <int DT>
__global__ __launch_bounds__(256) void kvzap_linear_kernel(ZapArgs a) {
    using T = typename Elem<DT>::T;
    __shared__ float red[4][ZL_TB][4][64];
    const uint32_t lane = threadIdx.x & 63, wv = uni((uint32_t)(threadIdx.x >> 6));
    const uint32_t n = lane & 15, kg = lane >> 4;
    const uint32_t t0 = blockIdx.x * ZL_TOK;
    const T* xr[ZL_TB];
#pragma unroll
    for (int tb = 0; tb < ZL_TB; ++tb) xr[tb] = zap_row<DT>(a, min(t0 + tb * 16 + n, a.R - 1)) + kg * 8;   // tokens past R: the last one (never stored)
    const bool has_w = n < (uint32_t)a.Hout;
    const T* wr = static_cast<const T*>(a.w1) + (int64_t)min(n, (uint32_t)a.Hout - 1) * a.K + kg * 8;
    f32x4 acc[ZL_TB];
#pragma unroll
    for (int tb = 0; tb < ZL_TB; ++tb) acc[tb] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto kstep = [&](uint32_t k) {
        const uint4 wf = has_w ? *reinterpret_cast<const uint4*>(wr + k) : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int tb = 0; tb < ZL_TB; ++tb) acc[tb] = mma16<DT>(wf, *reinterpret_cast<const uint4*>(xr[tb] + k), acc[tb]);
    };
    uint32_t k = wv * 32;
    for (; k + 3 * 128 < (uint32_t)a.K; k += 4 * 128) {   // four of this wave's k-steps: their loads in flight together
#pragma unroll
        for (int u = 0; u < 4; ++u) kstep(k + 128 * u);
    }
    for (; k < (uint32_t)a.K; k += 128) kstep(k);
#pragma unroll
    for (int tb = 0; tb < ZL_TB; ++tb)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) red[wv][tb][reg][lane] = acc[tb][reg];
    __syncthreads();
    // C: column lane & 15 = the token, row 4 (lane >> 4) + reg = the output; wave w finishes register w of every lane
    {
        const uint32_t reg = wv, o = 4 * kg + reg;
#pragma unroll
        for (int tb = 0; tb < ZL_TB; ++tb) {
            const uint32_t t = t0 + tb * 16 + n;
            const float sum = ((red[0][tb][reg][lane] + red[1][tb][reg][lane]) + red[2][tb][reg][lane]) + red[3][tb][reg][lane];
            if (t < a.R && o < (uint32_t)a.Hout) *zap_out(a, t, o) = sum + Elem<DT>::ld(static_cast<const T*>(a.b1) + o);
        }
    }
}

// ---- generic path: any dtype, alignment, K, N, Hout <= 256 (float32 modules, the tiny test models).  Correctness only: a wave per token,
// lane l owns elements l, l + 64, .. of the row; the hidden units one after the other, output o accumulated by lane o % 64.
constexpr int ZG_MAXQ = 4;
template <int DT>
__global__ __launch_bounds__(256) void kvzap_generic_kernel(ZapArgs a) {
    using T = typename Elem<DT>::T;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= a.R) return;
    const T* xr = zap_row<DT>(a, t);
    const T *w1 = static_cast<const T*>(a.w1), *b1 = static_cast<const T*>(a.b1);
    if (a.N == 0) {
        for (int o = 0; o < a.Hout; ++o) {
            float dot = 0.f;
            for (int k = lane; k < a.K; k += 64) dot = fmaf(Elem<DT>::ld(xr + k), Elem<DT>::ld(w1 + (int64_t)o * a.K + k), dot);
            dot = wave_sum(dot);
            if (lane == 0) *zap_out(a, t, o) = dot + Elem<DT>::ld(b1 + o);
        }
        return;
    }
    const T *w2 = static_cast<const T*>(a.w2), *b2 = static_cast<const T*>(a.b2);
    float p[ZG_MAXQ] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < a.N; ++j) {
        float dot = 0.f;
        for (int k = lane; k < a.K; k += 64) dot = fmaf(Elem<DT>::ld(xr + k), Elem<DT>::ld(w1 + (int64_t)j * a.K + k), dot);
        const float h = zap_gelu(wave_sum(dot) + Elem<DT>::ld(b1 + j));
#pragma unroll
        for (int q = 0; q < ZG_MAXQ; ++q) {
            const int o = lane + 64 * q;
            if (o < a.Hout) p[q] = fmaf(Elem<DT>::ld(w2 + (int64_t)o * a.N + j), h, p[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < ZG_MAXQ; ++q) {
        const int o = lane + 64 * q;
        if (o < a.Hout) *zap_out(a, t, o) = p[q] + Elem<DT>::ld(b2 + o);
    }
}

// ---- the paths and their launchers ----------------------------------------------------------------------------------------------------
enum { ZAP_AUTO = 0, ZAP_TILE = 1, ZAP_ROWS = 2, ZAP_GENERIC = 3 };   // KVP_KVZAP_PATH (A/B runs, the tests' path comparison)

bool zap_fast_ok(int dtype, const ZapArgs& a, int64_t K, int64_t Hout) {
    if (dtype == KVP_F32 || K % 32 != 0 || Hout > 16) return false;
    return (((uintptr_t)a.x | (uintptr_t)a.w1 | (uintptr_t)a.x_sb * 2 | (uintptr_t)a.x_ss * 2) & 15) == 0;
}
bool zap_tile_ok(int64_t N) { return N == 0 || (N % 32 == 0 && N >= 32 && N <= 1024); }
size_t zap_rows_slices(int64_t K, int64_t N, int64_t Hout, uint32_t* kslices) {
    const size_t ks = N > 0 ? 1 : (size_t)((K + ZR_KSLICE - 1) / ZR_KSLICE);
    if (kslices) *kslices = (uint32_t)ks;
    return (size_t)(((N > 0 ? N : Hout) + ZR_THREADS / 64 - 1) / (ZR_THREADS / 64)) * ks;
}

template <int DT, class Geo>
int zap_mfma_launch(const ZapArgs& a, hipStream_t st) {
    const size_t lds = Geo::lds_bytes(a.N, a.Hout);
    static bool raised = false;   // (per instantiation; raising twice is harmless)
    if (!raised) {
        const int rc = kvp_raise_dynamic_lds("kvp_kvzap_score", &kvzap_mfma_kernel<DT, Geo>, 160 * 1024);
        if (rc != KVP_OK) return rc;
        raised = true;
    }
    KVP_LAUNCH("kvzap_mfma", st, kvzap_mfma_kernel<DT, Geo><<<(a.R + Geo::TOK - 1) / Geo::TOK, Geo::THREADS, lds, st>>>(a));
    return KVP_OK;
}

template <int DT>
int zap_fast_run(const ZapArgs& a, int path, hipStream_t st) {
    if (path == ZAP_ROWS) {
        uint32_t ks;
        zap_rows_slices(a.K, a.N, a.Hout, &ks);
        const uint32_t fin = (a.R * a.Hout + 255) / 256;
        if (a.N > 0) {
            KVP_LAUNCH("kvzap_rows", st, kvzap_rows_kernel<DT, true><<<a.nslice, ZR_THREADS, 0, st>>>(a, ks));
            KVP_LAUNCH("kvzap_rows_finish", st, kvzap_rows_finish_kernel<DT, true><<<fin, 256, 0, st>>>(a, ks));
        } else {
            KVP_LAUNCH("kvzap_rows", st, kvzap_rows_kernel<DT, false><<<a.nslice, ZR_THREADS, 0, st>>>(a, ks));
            KVP_LAUNCH("kvzap_rows_finish", st, kvzap_rows_finish_kernel<DT, false><<<fin, 256, 0, st>>>(a, ks));
        }
        return KVP_OK;
    }
    if (a.N == 0) {
        KVP_LAUNCH("kvzap_linear", st, kvzap_linear_kernel<DT><<<(a.R + ZL_TOK - 1) / ZL_TOK, 256, 0, st>>>(a));
        return KVP_OK;
    }
    if (a.N <= 512) return zap_mfma_launch<DT, ZapGeo<2, 4, 64>>(a, st);
    return zap_mfma_launch<DT, ZapGeo<1, 8, 32>>(a, st);
}

// ---- kvp_threshold_*: the (b, h, position + shift) of every score < threshold in row-major order, two phases -----------------------------
// A block owns a chunk of 2048 positions of one (b, h) row, a thread 8 consecutive ones.  Phase 1: the chunks' counts, then their exclusive
// scan by one workgroup (int64) and the total.  Phase 2 recomputes the flags, ranks them inside the block (wave scan + the waves' totals) and
// writes at offset + rank: no atomics, the order is torch.where's.  The same kernels serve n = 1 and n = 131072.
constexpr int TS_THREADS = 256, TS_PER = 8, TS_CHUNK = TS_THREADS * TS_PER;

struct TsArgs {
    const float* sc;
    int64_t sb, sh, sn;
    uint32_t H, nch;   // heads; chunks per row
    int64_t n;
    float thr;
};

// exclusive scan of v over the block's threads (NW waves); total: the block's sum.  lds: NW words, free again on return
template <int NW> __device__ __forceinline__ uint32_t ts_block_scan(uint32_t v, uint32_t* lds, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
        if (lane >= (uint32_t)d) incl += up;
    }
    if (lane == 63) lds[wv] = incl;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const uint32_t x = lds[w];
        if ((uint32_t)w < wv) base += x;
        total += x;
    }
    __syncthreads();
    return base + incl - v;
}

// bit e: position chunk * 2048 + tid * 8 + e of the block's row exists and its score is below the threshold (a NaN is not)
__device__ __forceinline__ uint32_t ts_flags(const TsArgs& a, uint32_t row, uint32_t ch) {
    const uint32_t b = row / a.H, h = row - b * a.H;
    const float* r = a.sc + (int64_t)b * a.sb + (int64_t)h * a.sh;
    const int64_t p0 = (int64_t)ch * TS_CHUNK + threadIdx.x * TS_PER;
    uint32_t m = 0;
#pragma unroll
    for (int e = 0; e < TS_PER; ++e)
        if (p0 + e < a.n && r[(p0 + e) * a.sn] < a.thr) m |= 1u << e;
    return m;
}

__global__ __launch_bounds__(TS_THREADS) void ts_count_kernel(TsArgs a, uint32_t* counts) {
    __shared__ uint32_t lds[TS_THREADS / 64];
    const uint32_t row = blockIdx.x / a.nch, ch = blockIdx.x - row * a.nch;
    uint32_t total;
    ts_block_scan<TS_THREADS / 64>(__popc(ts_flags(a, row, ch)), lds, total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void ts_scan_kernel(const uint32_t* counts, uint32_t nblk, int64_t* offs, int64_t* total) {
    __shared__ uint32_t lds[16];
    int64_t base = 0;
    for (uint32_t i0 = 0; i0 < nblk; i0 += 1024) {   // (uniform trip count: the barriers inside are reached by every thread)
        const uint32_t i = i0 + threadIdx.x;
        const uint32_t v = i < nblk ? counts[i] : 0u;
        uint32_t sum;
        const uint32_t ex = ts_block_scan<16>(v, lds, sum);
        if (i < nblk) offs[i] = base + ex;
        base += sum;
    }
    if (threadIdx.x == 0) *total = base;
}

__global__ __launch_bounds__(TS_THREADS) void ts_fill_kernel(TsArgs a, const int64_t* offs, int64_t total, int64_t shift, int64_t* out_b,
                                                             int64_t* out_h, int64_t* out_p) {
    __shared__ uint32_t lds[TS_THREADS / 64];
    const uint32_t row = blockIdx.x / a.nch, ch = blockIdx.x - row * a.nch;
    const uint32_t m = ts_flags(a, row, ch);
    uint32_t sum;
    int64_t pos = offs[blockIdx.x] + ts_block_scan<TS_THREADS / 64>(__popc(m), lds, sum);
    const uint32_t b = row / a.H, h = row - b * a.H;
    const int64_t p0 = (int64_t)ch * TS_CHUNK + threadIdx.x * TS_PER;
#pragma unroll
    for (int e = 0; e < TS_PER; ++e) {
        if (((m >> e) & 1u) && pos >= 0 && pos < total) {   // (pos < total always, unless the scores changed between the phases)
            out_b[pos] = b;
            out_h[pos] = h;
            out_p[pos] = p0 + e + shift;
            ++pos;
        }
    }
}

struct TsWs {
    uint32_t* counts;
    int64_t *offs, *total;
    size_t bytes;
    TsWs(void* ws, size_t nblk) {
        KvpArena ar(ws);
        counts = ar.take<uint32_t>(nblk);
        offs = ar.take<int64_t>(nblk);
        total = ar.take<int64_t>(1);
        bytes = ar.bytes();
    }
};

// the shape checks both threshold entries share; nblk: blocks of either phase (0: nothing to do)
int ts_shape(const char* who, int64_t B, int64_t H, int64_t n, size_t* nblk) {
    KVP_CHECK_ARG(B >= 0 && H >= 0 && n >= 0 && B < ((int64_t)1 << 31) && H < ((int64_t)1 << 31) && n < ((int64_t)1 << 40), "%s: bad shape B=%lld H=%lld n=%lld",
                  who, (long long)B, (long long)H, (long long)n);
    const int64_t nch = (n + TS_CHUNK - 1) / TS_CHUNK;
    KVP_CHECK_ARG(B * H <= ((int64_t)1 << 31) / std::max<int64_t>(nch, 1) - 1, "%s: bad shape: too many chunks (B * H * ceil(n / %d))", who, TS_CHUNK);
    *nblk = (size_t)(B * H * nch);
    return KVP_OK;
}

TsArgs ts_args(const float* scores, int64_t sb, int64_t sh, int64_t sn, int64_t H, int64_t n, float threshold) {
    TsArgs a;
    a.sc = scores; a.sb = sb; a.sh = sh; a.sn = sn;
    a.H = (uint32_t)H; a.nch = (uint32_t)((n + TS_CHUNK - 1) / TS_CHUNK);
    a.n = n; a.thr = threshold;
    return a;
}

}  // namespace

// ================================================================================================================================
extern "C" size_t kvp_kvzap_score_workspace_bytes(int dtype, int64_t B, int64_t S, int64_t K, int64_t N, int64_t Hout) {
    (void)dtype;
    if (B < 1 || S < 1 || K < 1 || N < 0 || Hout < 1 || B * S > ZR_MAXR) return 0;   // only the few-rows path stores partials
    KvpArena ar(nullptr);
    ar.take<float>(zap_rows_slices(K, N, Hout, nullptr) * (size_t)(B * S) * (size_t)Hout);
    return ar.bytes();
}

extern "C" int kvp_kvzap_score(const void* x, int64_t x_sb, int64_t x_ss, int dtype, const void* w1, const void* b1, const void* w2,
                               const void* b2, int64_t B, int64_t S, int64_t K, int64_t N, int64_t Hout, float* out, int64_t o_sb,
                               int64_t o_sh, int64_t o_ss, void* ws, size_t ws_bytes, kvp_stream_t stream) {
    KVP_CHECK_DTYPE("kvp_kvzap_score", dtype);
    KVP_CHECK_ARG(B >= 1 && S >= 0 && K >= 1 && N >= 0 && Hout >= 1 && K < ((int64_t)1 << 24) && N < ((int64_t)1 << 24) && Hout <= 256 &&
                      S < ((int64_t)1 << 31) && B * S < ((int64_t)1 << 31) - 4096,
                  "kvp_kvzap_score: bad shape B=%lld S=%lld K=%lld N=%lld Hout=%lld", (long long)B, (long long)S, (long long)K, (long long)N,
                  (long long)Hout);
    if (S == 0) return KVP_OK;
    KVP_CHECK_ARG(x && w1 && b1 && out, "kvp_kvzap_score: null pointer");
    KVP_CHECK_ARG(N == 0 || (w2 && b2), "kvp_kvzap_score: null pointer (the second layer of an mlp, N = %lld)", (long long)N);
    hipStream_t st = (hipStream_t)stream;
    ZapArgs a;
    a.x = x; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2;
    a.x_sb = x_sb; a.x_ss = x_ss;
    a.S = (uint32_t)S; a.R = (uint32_t)(B * S);
    a.K = (int)K; a.N = (int)N; a.Hout = (int)Hout;
    a.out = out; a.o_sb = o_sb; a.o_sh = o_sh; a.o_ss = o_ss;
    a.part = nullptr; a.nslice = 0;

    const int knob = kvp_env_int("KVP_KVZAP_PATH", ZAP_AUTO);
    int path = ZAP_GENERIC;
    if (knob != ZAP_GENERIC && zap_fast_ok(dtype, a, K, Hout)) {
        const bool rows_ok = a.R <= (uint32_t)ZR_MAXR, tile_ok = zap_tile_ok(N);
        if (rows_ok && (knob != ZAP_TILE || !tile_ok)) path = ZAP_ROWS;
        else if (tile_ok) path = ZAP_TILE;
    }
    if (path == ZAP_ROWS) {
        uint32_t ks;
        a.nslice = (uint32_t)zap_rows_slices(K, N, Hout, &ks);
        KvpArena ar(ws);
        a.part = ar.take<float>((size_t)a.nslice * a.R * (size_t)Hout);
        const int rc = kvp_check_workspace("kvp_kvzap_score", ws, ws_bytes, ar.bytes());
        if (rc != KVP_OK) return rc;
    }
    if (path == ZAP_GENERIC) {
        KVP_DISPATCH_DTYPE(dtype, KVP_LAUNCH("kvzap_generic", st, kvzap_generic_kernel<DT><<<(a.R + 3) / 4, 256, 0, st>>>(a)));
    } else {
        const int rc = dtype == KVP_F16 ? zap_fast_run<KVP_F16>(a, path, st) : zap_fast_run<KVP_BF16>(a, path, st);
        if (rc != KVP_OK) return rc;
    }
    KVP_CHECK_LAUNCH("kvp_kvzap_score");
    return KVP_OK;
}

extern "C" size_t kvp_threshold_select_workspace_bytes(int64_t B, int64_t H, int64_t n) {
    if (B < 0 || H < 0 || n < 0) return 0;
    const size_t nch = (size_t)((n + TS_CHUNK - 1) / TS_CHUNK);
    return TsWs(nullptr, (size_t)B * (size_t)H * nch).bytes;
}

extern "C" int kvp_threshold_count(const float* scores, int64_t s_sb, int64_t s_sh, int64_t s_sn, int64_t B, int64_t H, int64_t n,
                                   float threshold, void* ws, size_t ws_bytes, int64_t* total, kvp_stream_t stream) {
    size_t nblk;
    int rc = ts_shape("kvp_threshold_count", B, H, n, &nblk);
    if (rc != KVP_OK) return rc;
    KVP_CHECK_ARG(total, "kvp_threshold_count: null pointer");
    *total = 0;
    if (nblk == 0) return KVP_OK;
    KVP_CHECK_ARG(scores, "kvp_threshold_count: null pointer");
    const TsWs w(ws, nblk);
    rc = kvp_check_workspace("kvp_threshold_count", ws, ws_bytes, w.bytes);
    if (rc != KVP_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const TsArgs a = ts_args(scores, s_sb, s_sh, s_sn, H, n, threshold);
    KVP_LAUNCH("threshold_count", st, ts_count_kernel<<<(uint32_t)nblk, TS_THREADS, 0, st>>>(a, w.counts));
    KVP_LAUNCH("threshold_scan", st, ts_scan_kernel<<<1, 1024, 0, st>>>(w.counts, (uint32_t)nblk, w.offs, w.total));
    KVP_CHECK_LAUNCH("kvp_threshold_count");
    // the one synchronisation of the selection: the reference's torch.where waits for its count in the same place
    hipError_t e = hipMemcpyAsync(total, w.total, sizeof(int64_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        kvp_set_error("kvp_threshold_count: reading the total failed: %s", hipGetErrorString(e));
        return KVP_EHIP;
    }
    return KVP_OK;
}

extern "C" int kvp_threshold_select(const float* scores, int64_t s_sb, int64_t s_sh, int64_t s_sn, int64_t B, int64_t H, int64_t n,
                                    float threshold, int64_t shift, const void* ws, size_t ws_bytes, int64_t total, int64_t* out_b,
                                    int64_t* out_h, int64_t* out_p, kvp_stream_t stream) {
    size_t nblk;
    int rc = ts_shape("kvp_threshold_select", B, H, n, &nblk);
    if (rc != KVP_OK) return rc;
    KVP_CHECK_ARG(total >= 0 && total <= B * H * n, "kvp_threshold_select: bad total %lld", (long long)total);
    if (nblk == 0 || total == 0) return KVP_OK;
    KVP_CHECK_ARG(scores && out_b && out_h && out_p, "kvp_threshold_select: null pointer");
    const TsWs w(const_cast<void*>(ws), nblk);
    rc = kvp_check_workspace("kvp_threshold_select", ws, ws_bytes, w.bytes);
    if (rc != KVP_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const TsArgs a = ts_args(scores, s_sb, s_sh, s_sn, H, n, threshold);
    KVP_LAUNCH("threshold_fill", st, ts_fill_kernel<<<(uint32_t)nblk, TS_THREADS, 0, st>>>(a, w.offs, total, shift, out_b, out_h, out_p));
    KVP_CHECK_LAUNCH("kvp_threshold_select");
    return KVP_OK;
}
