// FastKVzipPress's gate (kvpress/presses/fastkvzip_press.py:54-71) and the protected positions of :240-247 (include/kvpress_hip.h:
// kvp_fastkvzip_score).  With RMSNorm_g(v) = g * v / sqrt(mean(v^2) + eps) over vectors of D = 16:
//     q[s,h,g] = RMSNorm_gq(x[s] Wq^T + bq)     k[s,h] = RMSNorm_gk(x[s] Wk^T)
//     logit = <k, q_g> / sqrt(D) + b[h,g]       base_j = <k_base[h,j], q_g> / sqrt(D)
//     out[b,h,s] = mean_g 1 / (1 + sum_j exp(base_j - logit));   1.0f where s < protect_head or s >= S - protect_tail
// Nothing of extent S x columns is stored: a workgroup of the matrix-core kernel owns a tile of tokens and ALL (G + 1) * 16 projected
// columns of a group of kv heads, so both RMSNorms, the 1 + J dot products per query vector, the exps and the group mean run on its
// accumulators.  No atomics anywhere: every sum has one fixed order (d, then j, then g), runs are bit-identical.
//
// Geometry of the matrix-core kernel (kvzap.hip's tile loop: 8 waves, 128 tokens a workgroup, one workgroup a CU).  Heads are
// independent, so the grid is token tiles x head groups, a head group being the fewest equal parts of Hkv whose vectors fit, in one of two
// geometries: 512 weight rows = 32 vectors in K tiles of 64 (128 accumulator registers a lane), or 640 rows = 40 vectors in K tiles of 32
// (160 accumulator registers, 214 VGPRs, no spills; K tiles of 64 would need 192 KiB of LDS) -- the second where it saves a head group.
// Qwen3-8B (Hkv 8, G 4: 640 columns, K 4096, bf16), measured at 128k tokens (tools/fastkvzip_lab.py): one group of 8
// heads on 640 rows 0.931 ms a call; two groups of 4 heads on 512-row workgroups 0.996; four groups of 2 heads 1.402; eight groups of 1
// head 2.225.  Every further group re-reads x once more (1 MiB per 128 tokens next to the group's weight rows: 6 MiB per token tile for one
// group, 7 MiB for two) and shortens the MFMA run between barriers; with two groups of 4 heads the 10 row blocks also fall 3, 3, 2, 2 on
// the four column groups of waves, with one group of 8 they fall 5 each.  What bounds the call is kvp_kvzap_score's bound (kvzap.hip), a
// quarter longer: every workgroup streams its weight rows from the L2s, 6.1 GiB at 128k, 0.66 ms at the ~10 TB/s qproj.hip measured for
// the L2 -> CU path, against 0.27 ms at the bf16 matrix peak (the call reaches 0.29 of it, 1.42 x the vendor GEMM's time for the
// projections alone).  The epilogue is 17 dot products of 16 and 16 exps per query vector with no MFMA beside it.
#include <math.h>

#include "kvp_mfma.h"

namespace {

struct FkzArgs {
    const void *x, *wq, *bq, *wk, *b;
    const float *gq, *gk, *kbase;
    int64_t x_sb, x_ss;          // element strides of the hidden states [B, S, K]
    uint32_t S, R;               // R = B * S tokens (token t: b = t / S, s = t % S)
    int K, Hkv, G, D, J;
    int HG;                      // matrix-core path: kv heads per head group (blockIdx.y)
    float eps, dscale;           // dscale = sqrt(D)
    uint32_t head, tail_from;    // positions s < head or s >= tail_from are written as 1.0f
    float* out;                  // [B, Hkv, S] through element strides
    int64_t o_sb, o_sh, o_ss;
};

__device__ __forceinline__ void fkz_store(const FkzArgs& a, uint32_t t, uint32_t h, float v) {
    const uint32_t b = t / a.S, s = t - b * a.S;
    a.out[(int64_t)b * a.o_sb + (int64_t)h * a.o_sh + (int64_t)s * a.o_ss] = (s < a.head || s >= a.tail_from) ? 1.0f : v;
}
template <int DT> __device__ __forceinline__ const typename Elem<DT>::T* fkz_row(const FkzArgs& a, uint32_t t) {
    const uint32_t b = t / a.S, s = t - b * a.S;
    return static_cast<const typename Elem<DT>::T*>(a.x) + (int64_t)b * a.x_sb + (int64_t)s * a.x_ss;
}

// ---- matrix-core path: bf16 / f16, 16-byte aligned rows, K % 32 == 0, D == 16, J <= 16, G <= 8 ------------------------------------------
// The tile loop is kvzap.hip's: wave w owns the token group tg = w & 1 (TSUB blocks of 32 tokens) and the column group cg = w >> 1 (the
// 32-row blocks cb = cg + 4 j, j < NBW); acc[ts][j] = W block x X block^T, so lane (n, half) holds rows 32 cb + {0..3, 8..11, 16..19,
// 24..27} + 4 half of token n.  Which weight row lands in which LDS row is chosen so that those 16 rows are ONE vector: the group's
// vectors are numbered v = hl (G + 1) + j (j < G: query vector g = j of head h0 + hl, rows (h G + g) 16 .. of Wq; j == G: the head's key
// vector, rows h 16 .. of Wk), vector v sits in block v / 2 on the lane half v & 1, its element d in LDS row
// 32 (v / 2) + (d & 3) + 8 (d >> 2) + 4 (v & 1) -- accumulator register d.  Both RMSNorms are lane-local, no shuffles.  An odd number of
// vectors leaves the last block's upper half unused: it is requested clamped to the last vector and never read.
// An LDS tile is N weight rows followed by TOK token rows of KT elements, XOR-swizzled on the global side of the LDS-DMA (kvp_mfma.h),
// double-buffered.  Token rows past R are requested clamped to the last token (never stored); the K tail (K % 64 == 32, K tiles of 64)
// requests the chunks that exist and runs the k-steps that exist.
// Epilogue, in the LDS the tiles leave behind: bq, b, k_base and the norm weights as float32; every lane adds the bias and normalises
// its vectors in place; the key lanes put theirs into LDS; every query lane reads its token's key, does its 1 + J dot products (fma
// chains in d order), the exps and their sum in j order; the G partial scores of a (token, head) meet in LDS and are added in g order.
constexpr int FKZ_TOK = 128;   // tokens per workgroup, every geometry
template <int NBW_, int KT_> struct FkzGeo {
    static constexpr int THREADS = 512, WAVES = 8, CW = 4, TG = 2;
    static constexpr int TSUB = 2, NBW = NBW_, KT = KT_;
    static constexpr int TOK = TG * TSUB * 32;
    static_assert(TOK == FKZ_TOK, "fkz_kslot");
    static constexpr int NMAX = CW * NBW * 32, VMAX = NMAX / 16;   // weight rows and vectors a workgroup holds at most
    static constexpr int ROWB = KT * 2, CPR = ROWB / 16, RPW = 1024 / ROWB, KSTEPS = KT / 16;
    static constexpr int MAXG = ((NMAX + TOK) / RPW + WAVES - 1) / WAVES;   // row groups (one request each) a wave owns at most
    static __host__ __device__ __forceinline__ uint32_t sw(uint32_t row) { return CPR == 8 ? ((row >> 1) & 7u) : ((row >> 2) & 3u); }
    // floats of the epilogue's regions for `nh` heads: keys [nh, TOK, 16], k_base [nh, J, 16], b [nh, G], bias [nv, 16], norm weights
    // [2, 16], partial scores [nh G, TOK]
    static __host__ __device__ size_t epi_floats(int nh, int G, int J) {
        return (size_t)nh * TOK * 16 + (size_t)nh * J * 16 + (size_t)nh * G + (size_t)nh * (G + 1) * 16 + 32 + (size_t)nh * G * TOK;
    }
    static size_t lds_bytes(int HG, int G, int J) {
        const size_t nrows = (size_t)((HG * (G + 1) + 1) / 2) * 32;
        return std::max(2 * (nrows + TOK) * ROWB, epi_floats(HG, G, J) * 4);
    }
};

// the 16 floats of a key vector in LDS: the 16-byte chunk c of token tl sits in slot c ^ ((tl >> 2) & 3) of its 64 bytes, so the 16
// tokens of a read group hit 16 distinct slots of the 256-byte bank line
__device__ __forceinline__ float4* fkz_kslot(float* ks, uint32_t hl, uint32_t tl, uint32_t c) {
    return reinterpret_cast<float4*>(ks + ((size_t)hl * FKZ_TOK + tl) * 16 + ((c ^ ((tl >> 2) & 3u)) << 2));
}

template <int DT, class Geo>
__global__ __launch_bounds__(Geo::THREADS) void fastkvzip_mfma_kernel(FkzArgs a) {
    using T = typename Elem<DT>::T;
    extern __shared__ __attribute__((aligned(16))) unsigned char flds[];
    constexpr int TSUB = Geo::TSUB, NBW = Geo::NBW;
    const uint32_t lane = threadIdx.x & 63, wv = uni((uint32_t)(threadIdx.x >> 6));
    const uint32_t n = lane & 31, kg = lane >> 5;
    const uint32_t tg = wv & 1, cg = wv >> 1;
    const uint32_t K = (uint32_t)a.K, G = (uint32_t)a.G, G1 = G + 1, J = (uint32_t)a.J;
    const uint32_t h0 = blockIdx.y * (uint32_t)a.HG, nh = min((uint32_t)a.HG, (uint32_t)a.Hkv - h0);
    const uint32_t NV = nh * G1, NCB = (NV + 1) / 2, N = NCB * 32;
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
            const uint32_t rr = row & 31, d = (rr & 3) + 4 * (rr >> 3);
            const uint32_t v = min(2 * (row >> 5) + ((rr >> 2) & 1), NV - 1);   // the unused half of an odd last block: the last vector (never read)
            const uint32_t hl = v / G1, j = v - hl * G1, h = h0 + hl;
            const char* base = j < G ? static_cast<const char*>(a.wq) + ((int64_t)((h * G + j) * 16 + d) * K) * 2
                                     : static_cast<const char*>(a.wk) + ((int64_t)(h * 16 + d) * K) * 2;
            gptr[i] = base + chunk * 16;
        } else {
            const uint32_t t = min(tok0 + (row - N), a.R - 1);   // token rows past R: the last token (never stored)
            gptr[i] = reinterpret_cast<const char*>(fkz_row<DT>(a, t)) + chunk * 16;
        }
    }
    const uint32_t ldsbase = KVP_LDS_ADDR(flds);
    auto request_tile = [&](uint32_t kt, uint32_t buf_off) {
        const uint32_t k0 = kt * Geo::KT;
        const uint32_t nvc = min((uint32_t)Geo::CPR, (K - k0) / 8);   // 16-byte chunks of the row that exist in this tile
#pragma unroll
        for (int i = 0; i < Geo::MAXG; ++i) {
            const uint32_t g = wv + 8 * i;
            const uint32_t la = __builtin_amdgcn_readfirstlane(ldsbase + buf_off + min(g, ngroups - 1) * (Geo::RPW * Geo::ROWB));
            lds_dma16_if(g < ngroups && chunk_of[i] < nvc, la, gptr[i] + (int64_t)k0 * 2);
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
                    xf[ts] = *reinterpret_cast<const uint4*>(flds + bufc + row * Geo::ROWB + ((ch ^ Geo::sw(row)) << 4));
                }
#pragma unroll
                for (int j = 0; j < NBW; ++j) {
                    const uint32_t cb = cg + Geo::CW * j;
                    if (cb < NCB) {        // (wave-uniform)
                        const uint32_t row = cb * 32 + n;
                        const uint4 wf = *reinterpret_cast<const uint4*>(flds + bufc + row * Geo::ROWB + ((ch ^ Geo::sw(row)) << 4));
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
    float* ks = reinterpret_cast<float*>(flds);        // [nh, TOK, 16] (fkz_kslot)
    float* kbs = ks + nh * Geo::TOK * 16;               // [nh, J, 16]
    float* bs = kbs + nh * J * 16;                      // [nh, G]
    float* bqs = bs + nh * G;                           // [NV, 16] (zeros for the key vectors)
    float* gws = bqs + NV * 16;                         // gq [16], gk [16]
    float* red = gws + 32;                              // [nh G, TOK]
    for (uint32_t i = threadIdx.x; i < nh * J * 16; i += Geo::THREADS) kbs[i] = a.kbase[(size_t)h0 * J * 16 + i];
    for (uint32_t i = threadIdx.x; i < nh * G; i += Geo::THREADS) bs[i] = Elem<DT>::ld(static_cast<const T*>(a.b) + h0 * G + i);
    for (uint32_t i = threadIdx.x; i < NV * 16; i += Geo::THREADS) {
        const uint32_t v = i >> 4, hl = v / G1, j = v - hl * G1;
        bqs[i] = j < G ? Elem<DT>::ld(static_cast<const T*>(a.bq) + ((h0 + hl) * G + j) * 16 + (i & 15)) : 0.f;
    }
    if (threadIdx.x < 32) gws[threadIdx.x] = threadIdx.x < 16 ? a.gq[threadIdx.x] : a.gk[threadIdx.x - 16];
    __syncthreads();

    // bias, RMSNorm in place; the key vectors go to LDS
#pragma unroll
    for (int j = 0; j < NBW; ++j) {
        const uint32_t cb = cg + Geo::CW * j;
        if (cb < NCB) {
            const uint32_t v = 2 * cb + kg;
            const bool valid = v < NV;
            const uint32_t vv = min(v, NV - 1), hl = vv / G1, jj = vv - hl * G1;
            const bool isk = jj == G;
            float bb[16], gw[16];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 b4 = *reinterpret_cast<const float4*>(bqs + vv * 16 + 4 * q);
                const float4 g4 = *reinterpret_cast<const float4*>(gws + (isk ? 16 : 0) + 4 * q);
                bb[4 * q] = b4.x; bb[4 * q + 1] = b4.y; bb[4 * q + 2] = b4.z; bb[4 * q + 3] = b4.w;
                gw[4 * q] = g4.x; gw[4 * q + 1] = g4.y; gw[4 * q + 2] = g4.z; gw[4 * q + 3] = g4.w;
            }
#pragma unroll
            for (int ts = 0; ts < TSUB; ++ts) {
                float ss = 0.f;
#pragma unroll
                for (int d = 0; d < 16; ++d) {
                    const float e = acc[ts][j][d] + bb[d];
                    acc[ts][j][d] = e;
                    ss = fmaf(e, e, ss);
                }
                const float inv = 1.0f / sqrtf(ss * 0.0625f + a.eps);
#pragma unroll
                for (int d = 0; d < 16; ++d) acc[ts][j][d] = gw[d] * (acc[ts][j][d] * inv);
                if (valid && isk) {
                    const uint32_t tl = (tg * TSUB + ts) * 32 + n;
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        *fkz_kslot(ks, hl, tl, q) = make_float4(acc[ts][j][4 * q], acc[ts][j][4 * q + 1], acc[ts][j][4 * q + 2], acc[ts][j][4 * q + 3]);
                }
            }
        }
    }
    __syncthreads();

    // every query vector against its token's key and the head's sink keys
#pragma unroll
    for (int j = 0; j < NBW; ++j) {
        const uint32_t cb = cg + Geo::CW * j;
        if (cb < NCB) {
            const uint32_t v = 2 * cb + kg;
            const uint32_t vv = min(v, NV - 1), hl = vv / G1, jj = vv - hl * G1;
            if (v < NV && jj < G) {
                const float bias = bs[hl * G + jj];
#pragma unroll
                for (int ts = 0; ts < TSUB; ++ts) {
                    const uint32_t tl = (tg * TSUB + ts) * 32 + n;
                    float dot = 0.f;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float4 k4 = *fkz_kslot(ks, hl, tl, q);
                        dot = fmaf(k4.x, acc[ts][j][4 * q], dot);
                        dot = fmaf(k4.y, acc[ts][j][4 * q + 1], dot);
                        dot = fmaf(k4.z, acc[ts][j][4 * q + 2], dot);
                        dot = fmaf(k4.w, acc[ts][j][4 * q + 3], dot);
                    }
                    const float logit = dot / a.dscale + bias;
                    float sum = 0.f;
                    for (uint32_t jb = 0; jb < J; ++jb) {
                        const float* kb = kbs + (hl * J + jb) * 16;
                        float db = 0.f;
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const float4 k4 = *reinterpret_cast<const float4*>(kb + 4 * q);
                            db = fmaf(k4.x, acc[ts][j][4 * q], db);
                            db = fmaf(k4.y, acc[ts][j][4 * q + 1], db);
                            db = fmaf(k4.z, acc[ts][j][4 * q + 2], db);
                            db = fmaf(k4.w, acc[ts][j][4 * q + 3], db);
                        }
                        sum += expf(db / a.dscale - logit);
                    }
                    red[(hl * G + jj) * Geo::TOK + tl] = 1.0f / (1.0f + sum);
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < nh * Geo::TOK; e += Geo::THREADS) {
        const uint32_t hl = e / Geo::TOK, tl = e - hl * Geo::TOK, t = tok0 + tl;
        if (t < a.R) {
            float sum = red[(hl * G) * Geo::TOK + tl];
            for (uint32_t g = 1; g < G; ++g) sum += red[(hl * G + g) * Geo::TOK + tl];
            fkz_store(a, t, h0 + hl, sum / (float)G);
        }
    }
}

// ---- generic path: any dtype, alignment, K, D <= 64, any J and G with (G + 1) D <= 8192.  Correctness only: a wave per (token, head);
// every projected element is a lane-strided fma chain over K met by a butterfly; the vectors sit in LDS; lane v normalises vector v in d
// order, lane g does query vector g's dot products in d order and its exps in j order, lane 0 adds the G scores in g order.
constexpr int FG_MAXD = 64, FG_MAXVD = 8192;
template <int DT>
__global__ __launch_bounds__(64) void fastkvzip_generic_kernel(FkzArgs a) {
    using T = typename Elem<DT>::T;
    extern __shared__ __attribute__((aligned(16))) unsigned char flds[];
    float* vec = reinterpret_cast<float*>(flds);   // [G + 1, D]: the query vectors, then the key
    const uint32_t lane = threadIdx.x;
    const uint32_t t = blockIdx.x, h = blockIdx.y;
    const uint32_t K = (uint32_t)a.K, G = (uint32_t)a.G, D = (uint32_t)a.D, J = (uint32_t)a.J;
    const T* xr = fkz_row<DT>(a, t);
    for (uint32_t v = 0; v <= G; ++v) {
        for (uint32_t d = 0; d < D; ++d) {
            const int64_t wrow = v < G ? (int64_t)((h * G + v) * D + d) : (int64_t)(h * D + d);
            const T* wr = static_cast<const T*>(v < G ? a.wq : a.wk) + wrow * K;
            float dot = 0.f;
            for (uint32_t k = lane; k < K; k += 64) dot = fmaf(Elem<DT>::ld(xr + k), Elem<DT>::ld(wr + k), dot);
            dot = wave_sum(dot);
            if (lane == 0) vec[v * D + d] = v < G ? dot + Elem<DT>::ld(static_cast<const T*>(a.bq) + wrow) : dot;
        }
    }
    __syncthreads();
    for (uint32_t v = lane; v <= G; v += 64) {
        const float* gw = v < G ? a.gq : a.gk;
        float ss = 0.f;
        for (uint32_t d = 0; d < D; ++d) ss = fmaf(vec[v * D + d], vec[v * D + d], ss);
        const float inv = 1.0f / sqrtf(ss / (float)D + a.eps);
        for (uint32_t d = 0; d < D; ++d) vec[v * D + d] = gw[d] * (vec[v * D + d] * inv);
    }
    __syncthreads();
    for (uint32_t g = lane; g < G; g += 64) {
        const float *q = vec + g * D, *k = vec + G * D;
        float dot = 0.f;
        for (uint32_t d = 0; d < D; ++d) dot = fmaf(k[d], q[d], dot);
        const float logit = dot / a.dscale + Elem<DT>::ld(static_cast<const T*>(a.b) + h * G + g);
        float sum = 0.f;
        for (uint32_t jb = 0; jb < J; ++jb) {
            const float* kb = a.kbase + ((size_t)h * J + jb) * D;
            float db = 0.f;
            for (uint32_t d = 0; d < D; ++d) db = fmaf(kb[d], q[d], db);
            sum += expf(db / a.dscale - logit);
        }
        vec[g * D] = 1.0f / (1.0f + sum);   // (q_g is this lane's alone and no longer needed)
    }
    __syncthreads();
    if (lane == 0) {
        float sum = vec[0];
        for (uint32_t g = 1; g < G; ++g) sum += vec[g * D];
        fkz_store(a, t, h, sum / (float)G);
    }
}

// ---- the paths ------------------------------------------------------------------------------------------------------------------------
enum { FKZ_AUTO = 0, FKZ_TILE = 1, FKZ_GENERIC = 3 };   // KVP_FASTKVZIP_PATH (A/B runs, the tests' path comparison)

bool fkz_tile_ok(int dtype, const FkzArgs& a) {
    if (dtype == KVP_F32 || a.K % 32 != 0 || a.D != 16 || a.J > 16 || a.G > 8) return false;
    return (((uintptr_t)a.x | (uintptr_t)a.wq | (uintptr_t)a.wk | (uintptr_t)a.x_sb * 2 | (uintptr_t)a.x_ss * 2) & 15) == 0;
}

// kv heads per head group: the fewest equal parts of Hkv whose (G + 1) vectors a head fit the geometry's VMAX and whose epilogue fits the
// 160 KiB of LDS (KVP_FASTKVZIP_HEADS: fewer)
constexpr size_t FKZ_LDS_MAX = 160 * 1024;
template <class Geo> int fkz_heads_per_group(int Hkv, int G, int J) {
    int hmax = Geo::VMAX / (G + 1);
    while (hmax > 1 && Geo::lds_bytes(hmax, G, J) > FKZ_LDS_MAX) --hmax;
    const int parts = (Hkv + hmax - 1) / hmax;
    int hg = (Hkv + parts - 1) / parts;
    const int knob = kvp_env_int("KVP_FASTKVZIP_HEADS", 0);
    if (knob >= 1 && knob <= hmax) hg = std::min(knob, Hkv);
    return hg;
}

template <int DT, class Geo>
int fkz_tile_launch(FkzArgs a, hipStream_t st) {
    static bool raised = false;   // (per instantiation; raising twice is harmless)
    if (!raised) {
        const int rc = kvp_raise_dynamic_lds("kvp_fastkvzip_score", &fastkvzip_mfma_kernel<DT, Geo>, FKZ_LDS_MAX);
        if (rc != KVP_OK) return rc;
        raised = true;
    }
    a.HG = fkz_heads_per_group<Geo>(a.Hkv, a.G, a.J);
    const dim3 grid((a.R + Geo::TOK - 1) / Geo::TOK, (uint32_t)((a.Hkv + a.HG - 1) / a.HG));
    KVP_LAUNCH("fastkvzip_mfma", st, fastkvzip_mfma_kernel<DT, Geo><<<grid, Geo::THREADS, Geo::lds_bytes(a.HG, a.G, a.J), st>>>(a));
    return KVP_OK;
}

// 512 rows in K tiles of 64, or 640 rows in K tiles of 32 (160 accumulator registers) where that saves a head group
template <int DT>
int fkz_tile_run(const FkzArgs& a, hipStream_t st) {
    using Narrow = FkzGeo<4, 64>;
    using Wide = FkzGeo<5, 32>;
    const int hn = fkz_heads_per_group<Narrow>(a.Hkv, a.G, a.J), hw = fkz_heads_per_group<Wide>(a.Hkv, a.G, a.J);
    const int knob = kvp_env_int("KVP_FASTKVZIP_GEO", 0);   // 1: Narrow, 2: Wide (A/B runs)
    const bool wide = knob == 2 || (knob != 1 && (a.Hkv + hw - 1) / hw < (a.Hkv + hn - 1) / hn);
    return wide ? fkz_tile_launch<DT, Wide>(a, st) : fkz_tile_launch<DT, Narrow>(a, st);
}

}  // namespace

// ================================================================================================================================
extern "C" size_t kvp_fastkvzip_score_workspace_bytes(int dtype, int64_t B, int64_t S, int64_t K, int64_t Hkv, int64_t G, int64_t D, int64_t J) {
    (void)dtype; (void)B; (void)S; (void)K; (void)Hkv; (void)G; (void)D; (void)J;
    return 0;   // no path stores anything outside its workgroups' LDS
}

extern "C" int kvp_fastkvzip_score(const void* x, int64_t x_sb, int64_t x_ss, int dtype, const void* wq, const void* bq, const void* wk,
                                   const void* b, const float* gq, const float* gk, const float* k_base, int64_t B, int64_t S, int64_t K,
                                   int64_t Hkv, int64_t G, int64_t D, int64_t J, float eps, int64_t protect_head, int64_t protect_tail,
                                   float* out, int64_t o_sb, int64_t o_sh, int64_t o_ss, void* ws, size_t ws_bytes, kvp_stream_t stream) {
    (void)ws; (void)ws_bytes;   // reserved (include/kvpress_hip.h): no path needs scratch
    KVP_CHECK_DTYPE("kvp_fastkvzip_score", dtype);
    KVP_CHECK_ARG(D >= 1 && D <= FG_MAXD, "kvp_fastkvzip_score: bad output_dim D=%lld (1 .. %d)", (long long)D, FG_MAXD);
    KVP_CHECK_ARG(B >= 1 && S >= 0 && K >= 1 && Hkv >= 1 && G >= 1 && J >= 0 && K < ((int64_t)1 << 24) && Hkv <= 65535 && J < ((int64_t)1 << 16) &&
                      (G + 1) * D <= FG_MAXVD && S < ((int64_t)1 << 31) && B * S < ((int64_t)1 << 31) - 4096,
                  "kvp_fastkvzip_score: bad shape B=%lld S=%lld K=%lld Hkv=%lld G=%lld J=%lld", (long long)B, (long long)S, (long long)K,
                  (long long)Hkv, (long long)G, (long long)J);
    KVP_CHECK_ARG(protect_head >= 0 && protect_tail >= 0, "kvp_fastkvzip_score: bad protected counts head=%lld tail=%lld", (long long)protect_head,
                  (long long)protect_tail);
    KVP_CHECK_ARG(eps >= 0.f && eps == eps, "kvp_fastkvzip_score: bad eps %g", (double)eps);
    if (S == 0) return KVP_OK;
    KVP_CHECK_ARG(x && wq && bq && wk && b && gq && gk && out, "kvp_fastkvzip_score: null pointer");
    KVP_CHECK_ARG(J == 0 || k_base, "kvp_fastkvzip_score: null pointer (k_base with sink J = %lld)", (long long)J);
    hipStream_t st = (hipStream_t)stream;
    FkzArgs a;
    a.x = x; a.wq = wq; a.bq = bq; a.wk = wk; a.b = b;
    a.gq = gq; a.gk = gk; a.kbase = k_base;
    a.x_sb = x_sb; a.x_ss = x_ss;
    a.S = (uint32_t)S; a.R = (uint32_t)(B * S);
    a.K = (int)K; a.Hkv = (int)Hkv; a.G = (int)G; a.D = (int)D; a.J = (int)J;
    a.HG = 0;
    a.eps = eps; a.dscale = sqrtf((float)D);
    a.head = (uint32_t)std::min<int64_t>(protect_head, S);
    a.tail_from = (uint32_t)(S - std::min<int64_t>(protect_tail, S));
    a.out = out; a.o_sb = o_sb; a.o_sh = o_sh; a.o_ss = o_ss;

    const int knob = kvp_env_int("KVP_FASTKVZIP_PATH", FKZ_AUTO);
    if (knob != FKZ_GENERIC && fkz_tile_ok(dtype, a)) {
        const int rc = dtype == KVP_F16 ? fkz_tile_run<KVP_F16>(a, st) : fkz_tile_run<KVP_BF16>(a, st);
        if (rc != KVP_OK) return rc;
    } else {
        const dim3 grid(a.R, (uint32_t)Hkv);
        const size_t lds = (size_t)(G + 1) * D * sizeof(float);
        KVP_DISPATCH_DTYPE(dtype, KVP_LAUNCH("fastkvzip_generic", st, fastkvzip_generic_kernel<DT><<<grid, 64, lds, st>>>(a)));
    }
    KVP_CHECK_LAUNCH("kvp_fastkvzip_score");
    return KVP_OK;
}
