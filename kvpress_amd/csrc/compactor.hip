// The Compactor family's scorers (include/kvpress_hip.h: kvp_ncattn_score, kvp_leverage_score, kvp_compactor_combine):
//   * non-causal chunked attention column sums (non_causal_attention_press.py:47-122): per (b, kv head, chunk) one workgroup;
//     the chunk's logits never leave the CU (no [Hq, S, chunk] temporaries);
//   * approximate leverage scores on the pre-RoPE keys (leverage_press.py:47-110): mean, sketched Gram matrix, Cholesky with the
//     reference's jitter schedule (float64, one workgroup per head), x^T G^-1 x as ||L^-1 x||^2 with x recomputed from the keys;
//   * the global z-score both presses end with, and Compactor's blend + sink padding (compactor_press.py:87-122).
// Every reduction runs in a fixed order (no atomics): the scores are bit-identical from run to run.
#include <math.h>

#include <cstdlib>
#include <vector>

#include "kvp_mfma.h"

namespace {

constexpr int NC_THREADS = 512;   // MFMA path: 8 waves
constexpr int NC_WAVES = NC_THREADS / 64;
constexpr int GEN_THREADS = 256;  // generic paths
constexpr int ZS_BLOCKS = 256;    // partial sums of the global z-score
constexpr int LV_TILE = 32;       // tokens per leverage tile
constexpr int LV_THREADS = 256;

// block-wide sum / max of one value per thread, fixed order (wave butterflies, then the waves in index order); every thread gets it
template <int NT> __device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) s += red[i];
    return s;
}
template <int NT> __device__ __forceinline__ double block_sum_d(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);   // (written out: through a wave_sum call the scheduler moves the wave-index shift below)
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) s += red[i];
    return s;
}

// the logit the reference's softmax sees (non_causal_attention_press.py:88-91): the matmul output rounded to the model dtype; in the
// last chunk padded keys get -1e-9 (in the dtype) from every row, padded queries 0 from the valid keys
template <int DT> __device__ __forceinline__ float nc_logit(float acc, bool key_pad, bool query_pad) {
    return key_pad ? round_dt<DT>(-1e-9f) : (query_pad ? 0.f : round_dt<DT>(acc));
}

// ||v|| rounded to the model dtype (values.norm(dim=-1)), times the head-group mean of the column sums
template <int DT>
__device__ __forceinline__ float nc_vnorm(const typename Elem<DT>::T* vr, int D) {
    float s = 0.f;
    for (int d = 0; d < D; ++d) {
        const float x = Elem<DT>::ld(vr + d);
        s = fmaf(x, x, s);
    }
    return round_dt<DT>(sqrtf(s));
}

// ---- (a) MFMA path: bf16 / f16, D in {64, 96, 128, 256}, chunk % 32 == 0 and <= 512, G <= 16 --------------------------------------
// Workgroup = (chunk, kv head, b), 8 waves.  Per q-head g and block of QB query rows: the RoPE'd rows are staged in LDS (16-byte
// chunks XOR-swizzled by row); pass 1: a wave owns 32 query rows and walks the chunk's 32-key tiles (logits^T = K Q^T: a lane owns a
// query column, so the row max / sum stay in its registers) -> row max and 1 / sum in LDS; pass 2: a wave owns (key tile, query
// subset) pairs and recomputes the same logits, adding exp(l - m) / sum into 16 per-lane accumulators (keys in its registers).  After
// all heads: per pair a 32-lane butterfly over the query columns, the subsets summed in order through LDS, / G, times ||v||.
// Padding: padded keys and queries are zero rows here, so their logits are 0 where the reference writes -1e-9 (padded keys) or 0
// (padded queries).  exp(-1e-9 - m) and exp(0 - m) are the same float32 number for every row max m (1 - 1e-9 rounds to 1 and
// |m| >= 1e-9 absorbs it), as is the max itself to within 1e-9, so the softmax is the reference's without a per-element mask.
template <int D> struct NcGeo {
    static constexpr int CH = D / 8;                                    // 16-byte chunks per row
    static constexpr int QB = ((32768 / D) / 32) * 32 > 512 ? 512 : ((32768 / D) / 32) * 32;   // staged query rows (<= 64 KiB)
    static constexpr int KS = D / 16;                                   // MFMA k-steps
    static __device__ __forceinline__ int swz(int r, int c) { return c ^ (r & ((D % 128 == 0 || D == 64) ? 7 : 3)); }
};

template <int DT, int D>
__global__ __launch_bounds__(NC_THREADS) void ncattn_mfma_kernel(
    const typename Elem<DT>::T* __restrict__ q, int64_t q_sb, int q_sh, int q_ss,
    const typename Elem<DT>::T* __restrict__ cosp, const typename Elem<DT>::T* __restrict__ sinp, int64_t cs_sb, int cs_ss,
    const typename Elem<DT>::T* __restrict__ k, int64_t k_sb, int64_t k_sh, int k_ss,
    const typename Elem<DT>::T* __restrict__ v, int64_t v_sb, int64_t v_sh, int v_ss,
    int Hkv, int G, int S, int C, float* __restrict__ tmp) {
    using G_ = NcGeo<D>;
    using T = typename Elem<DT>::T;
    __shared__ __attribute__((aligned(16))) typename Elem<DT>::T qs[G_::QB * D];
    __shared__ float st_m[G_::QB];
    __shared__ float st_il[G_::QB];
    __shared__ float part[16 * 32];

    const int c = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
    const int c0 = c * C;
    const int nvalid = min(C, S - c0);
    const int nkt = C / 32;
    const int R = nkt >= NC_WAVES ? 1 : NC_WAVES / nkt;   // query subsets per key tile in pass 2
    const int npairs = nkt * R;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r32 = lane & 31, h = lane >> 5;
    const T* kb = k + (int64_t)b * k_sb + (int64_t)kvh * k_sh + (int64_t)c0 * k_ss;
    const T* qbase = q + (int64_t)b * q_sb + (int64_t)kvh * G * q_sh + (int64_t)c0 * q_ss;
    const T* cbase = cosp + (int64_t)b * cs_sb + (int64_t)c0 * cs_ss;
    const T* sbase = sinp + (int64_t)b * cs_sb + (int64_t)c0 * cs_ss;

    f32x16 colacc[2];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int i = 0; i < 16; ++i) colacc[p][i] = 0.f;

    for (int g = 0; g < G; ++g) {
        const T* qb = qbase + (int64_t)g * q_sh;
        for (int qb0 = 0; qb0 < C; qb0 += G_::QB) {
            const int nq = min(G_::QB, C - qb0);
            __syncthreads();   // the previous block's pass 2 is done with qs
            // stage RoPE'd rows: one thread per (row, d < D/2) pair, torch's per-op rounding (rope_elem)
            for (int idx = threadIdx.x; idx < nq * (D / 2); idx += NC_THREADS) {
                const int r = idx / (D / 2), d = idx % (D / 2);
                const int s = qb0 + r;   // within the chunk
                float lo = 0.f, hi = 0.f;
                if (s < nvalid) {
                    const T* qr = qb + s * q_ss;
                    const T* cr = cbase + s * cs_ss;
                    const T* sr = sbase + s * cs_ss;
                    const float q0 = Elem<DT>::ld(qr + d), q1 = Elem<DT>::ld(qr + d + D / 2);
                    lo = rope_elem<DT>(q0, Elem<DT>::ld(cr + d), -q1, Elem<DT>::ld(sr + d));
                    hi = rope_elem<DT>(q1, Elem<DT>::ld(cr + d + D / 2), q0, Elem<DT>::ld(sr + d + D / 2));
                }
                const int d2 = d + D / 2;
                qs[r * D + G_::swz(r, d / 8) * 8 + (d & 7)] = to_dt<DT>(lo);
                qs[r * D + G_::swz(r, d2 / 8) * 8 + (d2 & 7)] = to_dt<DT>(hi);
            }
            __syncthreads();
            // pass 1: row max and 1 / row sum
            for (int qt = wave; qt < nq / 32; qt += NC_WAVES) {
                const int row = qt * 32 + r32;
                uint4 bq[G_::KS];
#pragma unroll
                for (int s = 0; s < G_::KS; ++s) bq[s] = *reinterpret_cast<const uint4*>(&qs[row * D + G_::swz(row, 2 * s + h) * 8]);
                float m = -INFINITY, l = 0.f;
                for (int kt = 0; kt < nkt; ++kt) {
                    const int key = kt * 32 + r32;
                    f32x16 acc;
#pragma unroll
                    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
                    for (int s = 0; s < G_::KS; ++s) {
                        uint4 ak = make_uint4(0, 0, 0, 0);
                        if (key < nvalid) ak = *reinterpret_cast<const uint4*>(kb + key * k_ss + 16 * s + 8 * h);
                        acc = mma32<DT>(ak, bq[s], acc);
                    }
                    float x[16];
                    float tm = -INFINITY;
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        x[i] = round_acc<DT>(acc[i]);
                        tm = fmaxf(tm, x[i]);
                    }
                    const float mn = fmaxf(m, tm);
                    float ts = 0.f;
#pragma unroll
                    for (int i = 0; i < 16; ++i) ts += __expf(x[i] - mn);
                    l = l * __expf(m - mn) + ts;
                    m = mn;
                }
                const float mo = __shfl_xor(m, 32), lo = __shfl_xor(l, 32);
                const float mn = fmaxf(m, mo);
                // both halves combine in the same order (lower half first): identical in both lanes
                const float l0 = h == 0 ? l : lo, m0 = h == 0 ? m : mo, l1 = h == 0 ? lo : l, m1 = h == 0 ? mo : m;
                const float lt = l0 * __expf(m0 - mn) + l1 * __expf(m1 - mn);
                if (h == 0) {
                    st_m[row] = mn;
                    st_il[row] = 1.f / lt;
                }
            }
            __syncthreads();
            // pass 2: column sums of the normalised rows
#pragma unroll
            for (int pi = 0; pi < 2; ++pi) {
                const int p = wave + pi * NC_WAVES;
                if (p < npairs) {
                    const int kt = p % nkt, qsub = p / nkt;
                    const int key = kt * 32 + r32;
                    uint4 ak[G_::KS];
#pragma unroll
                    for (int s = 0; s < G_::KS; ++s) {
                        ak[s] = make_uint4(0, 0, 0, 0);
                        if (key < nvalid) ak[s] = *reinterpret_cast<const uint4*>(kb + key * k_ss + 16 * s + 8 * h);
                    }
                    for (int qt = qsub; qt < nq / 32; qt += R) {
                        const int row = qt * 32 + r32;
                        f32x16 acc;
#pragma unroll
                        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
                        for (int s = 0; s < G_::KS; ++s) {
                            const uint4 bq = *reinterpret_cast<const uint4*>(&qs[row * D + G_::swz(row, 2 * s + h) * 8]);
                            acc = mma32<DT>(ak[s], bq, acc);
                        }
                        const float mq = st_m[row], il = st_il[row];
#pragma unroll
                        for (int i = 0; i < 16; ++i) colacc[pi][i] += __expf(round_acc<DT>(acc[i]) - mq) * il;
                    }
                }
            }
        }
    }
    // reduce over the 32 query columns of each lane half, then over the query subsets in order
#pragma unroll
    for (int pi = 0; pi < 2; ++pi) {
        const int p = wave + pi * NC_WAVES;
        if (p < npairs) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                float x = colacc[pi][i];
#pragma unroll
                for (int o = 1; o < 32; o <<= 1) x += __shfl_xor(x, o);
                colacc[pi][i] = x;
            }
            if (r32 == 0) {
#pragma unroll
                for (int i = 0; i < 16; ++i) part[p * 32 + (i & 3) + 8 * (i >> 2) + 4 * h] = colacc[pi][i];
            }
        }
    }
    __syncthreads();
    const int j = threadIdx.x;
    if (j < nvalid) {
        const int kt = j / 32;
        float sum = 0.f;
        for (int r = 0; r < R; ++r) sum += part[(r * nkt + kt) * 32 + (j & 31)];
        const float vn = nc_vnorm<DT>(v + (int64_t)b * v_sb + (int64_t)kvh * v_sh + (int64_t)(c0 + j) * v_ss, D);
        tmp[((int64_t)b * Hkv + kvh) * S + c0 + j] = (sum / (float)G) * vn;   // (A / G) * ||v||
    }
}

// ---- (a) generic path: any dtype, head size and chunk (correct, slow) ----------------------------------------------------------
// Workgroup = (chunk, kv head, b); per query row: the RoPE'd row in LDS, two sweeps over the chunk's keys (row max / sum, then the
// normalised probabilities).  Key j's running column sum lives in tmp and is only ever touched by thread j % 256 of this workgroup.
template <int DT>
__global__ __launch_bounds__(GEN_THREADS) void ncattn_generic_kernel(
    const typename Elem<DT>::T* __restrict__ q, int64_t q_sb, int64_t q_sh, int64_t q_ss,
    const typename Elem<DT>::T* __restrict__ cosp, const typename Elem<DT>::T* __restrict__ sinp, int64_t cs_sb, int64_t cs_ss,
    const typename Elem<DT>::T* __restrict__ k, int64_t k_sb, int64_t k_sh, int64_t k_ss,
    const typename Elem<DT>::T* __restrict__ v, int64_t v_sb, int64_t v_sh, int64_t v_ss,
    int Hkv, int G, int S, int C, int D, float* __restrict__ tmp) {
    using T = typename Elem<DT>::T;
    extern __shared__ float qrow[];   // D floats
    __shared__ float red[GEN_THREADS / 64];
    const int c = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
    const int64_t c0 = (int64_t)c * C;
    const int nvalid = (int)min((int64_t)C, S - c0);
    const T* kb = k + (int64_t)b * k_sb + (int64_t)kvh * k_sh;
    float* out = tmp + ((int64_t)b * Hkv + kvh) * S;
    for (int j = threadIdx.x; j < nvalid; j += GEN_THREADS) out[c0 + j] = 0.f;
    for (int g = 0; g < G; ++g) {
        const int hq = kvh * G + g;
        for (int i = 0; i < C; ++i) {
            const int64_t s = c0 + i;
            const bool qpad = i >= nvalid;
            __syncthreads();
            for (int d = threadIdx.x; d < D / 2; d += GEN_THREADS) {
                float lo = 0.f, hi = 0.f;
                if (!qpad) {
                    const T* qr = q + (int64_t)b * q_sb + (int64_t)hq * q_sh + s * q_ss;
                    const T* cr = cosp + (int64_t)b * cs_sb + s * cs_ss;
                    const T* sr = sinp + (int64_t)b * cs_sb + s * cs_ss;
                    const float q0 = Elem<DT>::ld(qr + d), q1 = Elem<DT>::ld(qr + d + D / 2);
                    lo = rope_elem<DT>(q0, Elem<DT>::ld(cr + d), -q1, Elem<DT>::ld(sr + d));
                    hi = rope_elem<DT>(q1, Elem<DT>::ld(cr + d + D / 2), q0, Elem<DT>::ld(sr + d + D / 2));
                }
                qrow[d] = lo;
                qrow[d + D / 2] = hi;
            }
            __syncthreads();
            float m = -INFINITY, l = 0.f;
            for (int j = threadIdx.x; j < C; j += GEN_THREADS) {
                float acc = 0.f;
                if (j < nvalid)
                    for (int d = 0; d < D; ++d) acc = fmaf(qrow[d], Elem<DT>::ld(kb + (c0 + j) * k_ss + d), acc);
                const float x = nc_logit<DT>(acc, j >= nvalid, qpad);
                const float mn = fmaxf(m, x);
                l = l * __expf(m - mn) + __expf(x - mn);
                m = mn;
            }
            // combine (m, l) over the block in a fixed order: the block max first, then the rescaled sums
            float mx = m;
            {
                mx = wave_max(mx);
                __syncthreads();
                if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
                __syncthreads();
                mx = red[0];
#pragma unroll
                for (int w = 1; w < GEN_THREADS / 64; ++w) mx = fmaxf(mx, red[w]);
            }
            const float lt = block_sum<GEN_THREADS>(m == -INFINITY ? 0.f : l * __expf(m - mx), red);
            const float il = 1.f / lt;
            for (int j = threadIdx.x; j < nvalid; j += GEN_THREADS) {
                float acc = 0.f;
                for (int d = 0; d < D; ++d) acc = fmaf(qrow[d], Elem<DT>::ld(kb + (c0 + j) * k_ss + d), acc);
                out[c0 + j] += __expf(nc_logit<DT>(acc, false, qpad) - mx) * il;
            }
        }
    }
    for (int j = threadIdx.x; j < nvalid; j += GEN_THREADS) {
        const float vn = nc_vnorm<DT>(v + (int64_t)b * v_sb + (int64_t)kvh * v_sh + (c0 + j) * v_ss, D);
        out[c0 + j] = (out[c0 + j] / (float)G) * vn;
    }
}

// ---- global z-score: (x - mean) / max(std, 1e-6) over the whole [B, H, S] tensor (non_causal_attention_press.py:121) -----------
// zs_sum: optional avg_pool1d(3, pad 1, count_include_pad) of each row of `in` into `out` (else out = in), partial sums per block;
// zs_sqdev: the mean from the partials (every block in the same order), partial sums of squared deviations; zs_apply.
__global__ __launch_bounds__(GEN_THREADS) void zs_sum_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t n, int64_t S,
                                                             int pool, double* __restrict__ part) {
    __shared__ double red[GEN_THREADS / 64];
    const int64_t per = (n + ZS_BLOCKS - 1) / ZS_BLOCKS;
    const int64_t lo = blockIdx.x * per, hi = min(n, lo + per);
    double acc = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += GEN_THREADS) {
        float x = in[i];
        if (pool) {
            const int64_t s = i % S;
            float a = s > 0 ? in[i - 1] : 0.f;
            a = __fadd_rn(a, x);
            a = __fadd_rn(a, s + 1 < S ? in[i + 1] : 0.f);
            x = a / 3.f;
            out[i] = x;
        } else if (out != in) {
            out[i] = x;
        }
        acc += (double)x;
    }
    const double t = block_sum_d<GEN_THREADS>(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

__device__ __forceinline__ double zs_total(const double* part) {
    double s = 0.0;
    for (int i = 0; i < ZS_BLOCKS; ++i) s += part[i];
    return s;
}

__global__ __launch_bounds__(GEN_THREADS) void zs_sqdev_kernel(const float* __restrict__ x, int64_t n, const double* __restrict__ part,
                                                               double* __restrict__ part2) {
    __shared__ double red[GEN_THREADS / 64];
    const float mean = (float)(zs_total(part) / (double)n);
    const int64_t per = (n + ZS_BLOCKS - 1) / ZS_BLOCKS;
    const int64_t lo = blockIdx.x * per, hi = min(n, lo + per);
    double acc = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += GEN_THREADS) {
        const double d = (double)x[i] - (double)mean;
        acc += d * d;
    }
    const double t = block_sum_d<GEN_THREADS>(acc, red);
    if (threadIdx.x == 0) part2[blockIdx.x] = t;
}

__global__ __launch_bounds__(GEN_THREADS) void zs_apply_kernel(const float* __restrict__ x, int64_t n, const double* __restrict__ part,
                                                               const double* __restrict__ part2, float* __restrict__ z) {
    const float mean = (float)(zs_total(part) / (double)n);
    // torch: the unbiased std of ONE element is NaN, and clamp_min keeps a NaN (fmaxf would drop it)
    const float sd = n > 1 ? fmaxf((float)sqrt(zs_total(part2) / (double)(n - 1)), 1e-6f) : __int_as_float(0x7fc00000);
    for (int64_t i = blockIdx.x * (int64_t)GEN_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * GEN_THREADS)
        z[i] = __fsub_rn(x[i], mean) / sd;
}

// ---- (b) leverage scores -----------------------------------------------------------------------------------------------------
// lv_mean: per (b, h) and token range, the sum over tokens of each dimension (partials, summed in order by the next kernels).
template <int DT>
__global__ __launch_bounds__(LV_THREADS) void lv_mean_kernel(const typename Elem<DT>::T* __restrict__ k, int64_t k_sb, int64_t k_sh,
                                                             int64_t k_ss, int H, int S, int D, int nb, float* __restrict__ mpart) {
    __shared__ float red[LV_THREADS];
    const int bh = blockIdx.y, b = bh / H, h = bh % H;
    const int rows = LV_THREADS / D;   // D <= 256
    const int d = threadIdx.x % D, r = threadIdx.x / D;
    const int per = (S + nb - 1) / nb;
    const int lo = blockIdx.x * per, hi = min(S, lo + per);
    const typename Elem<DT>::T* kb = k + (int64_t)b * k_sb + (int64_t)h * k_sh;
    float acc = 0.f;
    if (r < rows)
        for (int s = lo + r; s < hi; s += rows) acc += Elem<DT>::ld(kb + (int64_t)s * k_ss + d);
    red[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x < D) {
        float t = 0.f;
        for (int i = 0; i < rows; ++i) t += red[i * D + threadIdx.x];
        mpart[((int64_t)bh * nb + blockIdx.x) * D + threadIdx.x] = t;
    }
}

// x = Phi^T (k - mu) for LV_TILE tokens from t0 into xs[LV_TILE][ks + 1] (padded rows); mu (model dtype, rounded as keys.mean() is) in
// mu_s, the centred rows in xc, Phi from LDS (phis) or, when it does not fit there, from global memory.  Tokens >= S give x = 0.
template <int DT>
__device__ __forceinline__ void lv_sketch_tile(const typename Elem<DT>::T* kb, int64_t k_ss, const typename Elem<DT>::T* pb, int64_t p_sd,
                                               int S, int D, int ks, int t0, const float* mu_s, float* xc, float* xs,
                                               const float* phis) {
    for (int i = threadIdx.x; i < LV_TILE * D; i += LV_THREADS) {
        const int t = i / D, d = i % D;
        float x = 0.f;
        if (t0 + t < S) x = round_dt<DT>(__fsub_rn(Elem<DT>::ld(kb + (int64_t)(t0 + t) * k_ss + d), mu_s[d]));
        xc[i] = x;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < LV_TILE * ks; i += LV_THREADS) {
        const int t = i / ks, j = i % ks;
        float acc = 0.f;
        if (phis)
            for (int d = 0; d < D; ++d) acc = fmaf(xc[t * D + d], phis[d * ks + j], acc);
        else
            for (int d = 0; d < D; ++d) acc = fmaf(xc[t * D + d], Elem<DT>::ld(pb + (int64_t)d * p_sd + j), acc);
        xs[t * (ks + 1) + j] = t0 + t < S ? round_dt<DT>(acc) : 0.f;
    }
    __syncthreads();
}

// the sketch of the head in LDS (float) when it fits in LV_PHI_LDS floats, else nullptr (read from global)
constexpr int LV_PHI_LDS = 8192;
template <int DT>
__device__ __forceinline__ const float* lv_load_phi(const typename Elem<DT>::T* pb, int64_t p_sd, int D, int ks, float* phis) {
    if (D * ks > LV_PHI_LDS) return nullptr;
    for (int i = threadIdx.x; i < D * ks; i += LV_THREADS) phis[i] = Elem<DT>::ld(pb + (int64_t)(i / ks) * p_sd + i % ks);
    __syncthreads();
    return phis;
}

template <int DT>
__device__ __forceinline__ void lv_load_mu(const float* mpart, int64_t bh, int nb, int S, int D, float* mu_s) {
    for (int d = threadIdx.x; d < D; d += LV_THREADS) {
        float s = 0.f;
        for (int i = 0; i < nb; ++i) s += mpart[(bh * nb + i) * D + d];
        mu_s[d] = round_dt<DT>(s / (float)S);
    }
    __syncthreads();
}

// lv_gram: grid (token blocks, B*H, RB-row blocks of G): partial G rows [RB rb, RB rb + RB) x all columns over the block's tiles;
// NU = entries per thread (compile time: the accumulators stay in registers)
template <int DT, int NU>
__global__ __launch_bounds__(LV_THREADS) void lv_gram_kernel(const typename Elem<DT>::T* __restrict__ k, int64_t k_sb, int64_t k_sh,
                                                             int64_t k_ss, const typename Elem<DT>::T* __restrict__ phi, int64_t p_sb,
                                                             int64_t p_sh, int64_t p_sd, int H, int S, int D, int ks, int nb,
                                                             const float* __restrict__ mpart, int nb2, int RB, float* __restrict__ gpart) {
    __shared__ float mu_s[256];
    __shared__ float xc[LV_TILE * 256];
    __shared__ float xs[LV_TILE * 257];
    __shared__ float phis_s[LV_PHI_LDS];
    const int bh = blockIdx.y, b = bh / H, h = bh % H, rb = blockIdx.z;
    const typename Elem<DT>::T* kb = k + (int64_t)b * k_sb + (int64_t)h * k_sh;
    const typename Elem<DT>::T* pb = phi + (int64_t)b * p_sb + (int64_t)h * p_sh;
    const float* phis = lv_load_phi<DT>(pb, p_sd, D, ks, phis_s);
    lv_load_mu<DT>(mpart, bh, nb, S, D, mu_s);
    const int ntiles = (S + LV_TILE - 1) / LV_TILE;
    const int per = (ntiles + nb2 - 1) / nb2;
    const int tlo = blockIdx.x * per, thi = min(ntiles, tlo + per);
    const int nent = RB * ks;   // entries of this row block (rows past ks are skipped)
    float acc[NU];
    int ij[NU];   // (i << 16) | j of each owned entry (entries past the matrix compute x_0 x_0 and are not stored)
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        acc[u] = 0.f;
        const int e = threadIdx.x + u * LV_THREADS;
        const int i = RB * rb + e / ks, j = e % ks;
        ij[u] = (e < nent && i < ks) ? ((i << 16) | j) : 0;
    }
    for (int tt = tlo; tt < thi; ++tt) {
        lv_sketch_tile<DT>(kb, k_ss, pb, p_sd, S, D, ks, tt * LV_TILE, mu_s, xc, xs, phis);
#pragma unroll 1
        for (int t = 0; t < LV_TILE; ++t) {
            const float* xt = xs + t * (ks + 1);
#pragma unroll
            for (int u = 0; u < NU; ++u) acc[u] = fmaf(xt[ij[u] >> 16], xt[ij[u] & 0xffff], acc[u]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int e = threadIdx.x + u * LV_THREADS;
        if (e < nent && RB * rb + e / ks < ks)
            gpart[(((int64_t)bh * nb2 + blockIdx.x) * ks + (ij[u] >> 16)) * ks + (ij[u] & 0xffff)] = acc[u];
    }
}

// lv_chol: one workgroup per head.  G = sum of the partials (in order), symmetrised in float32 (0.5 * (G + G^T)), then Cholesky of
// G + jitter I in float64 with jitter 1e-2, x10, at most 5 tries (leverage_press.py:47-56, :90); minv = L^-1 (float32).  A head whose
// last try fails gets status 1 and NaN in minv (kvp_leverage_status turns that into an error).
__global__ __launch_bounds__(LV_THREADS) void lv_chol_kernel(const float* __restrict__ gpart, int nb2, int ks, double* __restrict__ A,
                                                             double* __restrict__ Y, float* __restrict__ minv, int* __restrict__ status) {
    __shared__ int fail;
    const int64_t bh = blockIdx.x;
    const int64_t kk = (int64_t)ks * ks;
    double* a = A + bh * kk;
    double* y = Y + bh * kk;
    float* mi = minv + bh * kk;
    double jitter = 1e-2;
    bool ok = false;
    for (int attempt = 0; attempt < 5 && !ok; ++attempt) {
        for (int e = threadIdx.x; e < kk; e += LV_THREADS) {
            const int i = e / ks, j = e % ks;
            float gij = 0.f, gji = 0.f;
            for (int p = 0; p < nb2; ++p) {
                gij += gpart[((bh * nb2 + p) * ks + i) * ks + j];
                gji += gpart[((bh * nb2 + p) * ks + j) * ks + i];
            }
            float s = 0.5f * __fadd_rn(gij, gji);
            if (i == j) s = __fadd_rn(s, (float)jitter);
            a[e] = (double)s;
        }
        if (threadIdx.x == 0) fail = 0;
        __syncthreads();
        for (int j = 0; j < ks; ++j) {
            if (threadIdx.x == 0) {
                const double dj = a[(int64_t)j * ks + j];
                if (!(dj > 0.0)) fail = 1;
                else a[(int64_t)j * ks + j] = sqrt(dj);
            }
            __syncthreads();
            if (fail) break;
            const double ljj = a[(int64_t)j * ks + j];
            for (int i = j + 1 + threadIdx.x; i < ks; i += LV_THREADS) a[(int64_t)i * ks + j] /= ljj;
            __syncthreads();
            const int m = ks - j - 1;
            for (int e = threadIdx.x; e < m * m; e += LV_THREADS) {
                const int i = j + 1 + e / m, l = j + 1 + e % m;
                if (l <= i) a[(int64_t)i * ks + l] -= a[(int64_t)i * ks + j] * a[(int64_t)l * ks + j];
            }
            __syncthreads();
        }
        ok = !fail;
        __syncthreads();
        jitter *= 10.0;
    }
    // L^-1, one column per thread: forward substitution
    for (int col = threadIdx.x; col < ks; col += LV_THREADS) {
        for (int i = 0; i < ks; ++i) {
            double v = 0.0;
            if (i >= col) {
                v = i == col ? 1.0 : 0.0;
                for (int m2 = col; m2 < i; ++m2) v -= a[(int64_t)i * ks + m2] * y[(int64_t)m2 * ks + col];
                v /= a[(int64_t)i * ks + i];
            }
            y[(int64_t)i * ks + col] = v;
            mi[(int64_t)i * ks + col] = ok ? (float)v : __int_as_float(0x7fc00000);
        }
    }
    if (threadIdx.x == 0) status[bh] = ok ? 0 : 1;
}

// lv_score: per tile of tokens (a block walks tiles blockIdx.x, + gridDim.x, ...), x recomputed from the keys (Phi from global memory:
// staging it in LDS per block measured slower here, 5.3 against 2.2 ms at 128k), score = ||L^-1 x||^2 (= x^T G^-1 x, leverage_press.py:100-109), >= 0
template <int DT>
__global__ __launch_bounds__(LV_THREADS) void lv_score_kernel(const typename Elem<DT>::T* __restrict__ k, int64_t k_sb, int64_t k_sh,
                                                              int64_t k_ss, const typename Elem<DT>::T* __restrict__ phi, int64_t p_sb,
                                                              int64_t p_sh, int64_t p_sd, int H, int S, int D, int ks, int nb,
                                                              const float* __restrict__ mpart, const float* __restrict__ minv,
                                                              float* __restrict__ raw) {
    __shared__ float mu_s[256];
    __shared__ float xc[LV_TILE * 256];
    __shared__ float xs[LV_TILE * 257];
    __shared__ float red[LV_THREADS];
    const int bh = blockIdx.y, b = bh / H, h = bh % H;
    const typename Elem<DT>::T* kb = k + (int64_t)b * k_sb + (int64_t)h * k_sh;
    const typename Elem<DT>::T* pb = phi + (int64_t)b * p_sb + (int64_t)h * p_sh;
    lv_load_mu<DT>(mpart, bh, nb, S, D, mu_s);
    const float* mb = minv + (int64_t)bh * ks * ks;
    const int t = threadIdx.x & (LV_TILE - 1), grp = threadIdx.x / LV_TILE;   // 8 row groups
    const int ntiles = (S + LV_TILE - 1) / LV_TILE;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int t0 = tile * LV_TILE;
        lv_sketch_tile<DT>(kb, k_ss, pb, p_sd, S, D, ks, t0, mu_s, xc, xs, nullptr);
        const float* xt = xs + t * (ks + 1);
        float acc = 0.f;
        for (int i = grp; i < ks; i += LV_THREADS / LV_TILE) {
            float yi = 0.f;
            for (int j = 0; j <= i; ++j) yi = fmaf(mb[(int64_t)i * ks + j], xt[j], yi);
            acc = fmaf(yi, yi, acc);
        }
        red[threadIdx.x] = acc;
        __syncthreads();
        if (threadIdx.x < LV_TILE && t0 + threadIdx.x < S) {
            float sc = 0.f;
            for (int g = 0; g < LV_THREADS / LV_TILE; ++g) sc += red[g * LV_TILE + threadIdx.x];
            raw[(int64_t)bh * S + t0 + threadIdx.x] = sc != sc ? sc : fmaxf(sc, 0.f);
        }
        __syncthreads();
    }
}

// ---- (c) Compactor: blending * z_lev + z_attn, sinks padded with the global max (compactor_press.py:114-122) ---------------------
// max that propagates NaN, as torch's Tensor.max() does (z-scores of a single-token middle are NaN in the reference)
__device__ __forceinline__ float cpt_nanmax(float a, float b) { return (a != a || b != b) ? __int_as_float(0x7fc00000) : fmaxf(a, b); }
__global__ __launch_bounds__(GEN_THREADS) void cpt_blend_kernel(const float* __restrict__ zl, const float* __restrict__ za, int64_t R,
                                                                int64_t Si, int64_t left, int64_t right, float blending,
                                                                float* __restrict__ out, float* __restrict__ pmax) {
    __shared__ float red[GEN_THREADS / 64];
    const int64_t n = R * Si, So = Si + left + right;
    const int64_t per = (n + ZS_BLOCKS - 1) / ZS_BLOCKS;
    const int64_t lo = blockIdx.x * per, hi = min(n, lo + per);
    float m = -INFINITY;
    for (int64_t i = lo + threadIdx.x; i < hi; i += GEN_THREADS) {
        const int64_t r = i / Si, s = i % Si;
        const float x = __fadd_rn(__fmul_rn(blending, zl[i]), za[i]);
        out[r * So + left + s] = x;
        m = cpt_nanmax(m, x);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = cpt_nanmax(m, __shfl_xor(m, o));   // (written out, as block_sum_d's ladder: a shared butterfly changes the code around it)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = red[0];
        for (int w = 1; w < GEN_THREADS / 64; ++w) t = cpt_nanmax(t, red[w]);
        pmax[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(GEN_THREADS) void cpt_pad_kernel(int64_t R, int64_t Si, int64_t left, int64_t right, const float* __restrict__ pmax,
                                                              float* __restrict__ out) {
    float m = -INFINITY;
    for (int i = 0; i < ZS_BLOCKS; ++i) m = cpt_nanmax(m, pmax[i]);
    const int64_t ns = left + right, So = Si + ns;
    for (int64_t i = blockIdx.x * (int64_t)GEN_THREADS + threadIdx.x; i < R * ns; i += (int64_t)gridDim.x * GEN_THREADS) {
        const int64_t r = i / ns, s = i % ns;
        out[r * So + (s < left ? s : Si + s)] = m;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
struct ZsWs {
    double* part;
    double* part2;
};
ZsWs zs_take(KvpArena& ar) {
    double* p = ar.take<double>(2 * ZS_BLOCKS);
    return {p, p + ZS_BLOCKS};
}

int zscore_launch(const float* in, float* raw, int64_t n, int64_t S, int pool, float* z, ZsWs w, hipStream_t st) {
    KVP_LAUNCH("cpt_zs_sum", st, zs_sum_kernel<<<ZS_BLOCKS, GEN_THREADS, 0, st>>>(in, raw, n, S, pool, w.part));
    KVP_CHECK_LAUNCH("zs_sum_kernel");
    KVP_LAUNCH("cpt_zs_sqdev", st, zs_sqdev_kernel<<<ZS_BLOCKS, GEN_THREADS, 0, st>>>(raw, n, w.part, w.part2));
    KVP_CHECK_LAUNCH("zs_sqdev_kernel");
    const int64_t nb = std::min<int64_t>((n + GEN_THREADS - 1) / GEN_THREADS, 4096);
    KVP_LAUNCH("cpt_zs_apply", st, zs_apply_kernel<<<(unsigned)std::max<int64_t>(nb, 1), GEN_THREADS, 0, st>>>(raw, n, w.part, w.part2, z));
    KVP_CHECK_LAUNCH("zs_apply_kernel");
    return KVP_OK;
}

// non-causal attention workspace
struct NcWs {
    float *tmp, *raw;   // [B*Hkv*S] each
    ZsWs zs;
    size_t total;
};
NcWs nc_ws(void* ws, int64_t B, int64_t Hkv, int64_t S) {
    NcWs w;
    KvpArena ar(ws);
    w.tmp = ar.take<float>((size_t)(B * Hkv * S));
    w.raw = ar.take<float>((size_t)(B * Hkv * S));
    w.zs = zs_take(ar);
    w.total = ar.bytes();
    return w;
}

// the tensors and sizes of one kvp_ncattn_score call
struct NcCall {
    KvpRows q, k, v;
    KvpRope r;
    int Hkv, G, S, C, D;
    float* tmp;
};

// KVP_NCATTN_GENERIC=1 sends every shape to the generic kernel (tests of that path on the shapes the MFMA kernel takes)
bool nc_mfma_ok(const NcCall& c, int dtype) {
    if (dtype == KVP_F32 || c.G > 16 || c.C % 32 != 0 || c.C > 512) return false;
    if (!(c.D == 64 || c.D == 96 || c.D == 128 || c.D == 256)) return false;
    if (kvp_env_int("KVP_NCATTN_GENERIC", 0)) return false;
    // row / head strides as 32-bit numbers inside the kernel (one chunk of rows from a per-block base pointer)
    const int64_t lim = (int64_t)1 << 30, C = c.C;
    if (std::abs(c.q.sh) * 16 >= lim || std::abs(c.q.ss) * C >= lim || std::abs(c.r.sw) * C >= lim || std::abs(c.k.ss) * C >= lim || std::abs(c.v.ss) >= lim)
        return false;
    // 16-byte key fragments straight from the cache rows
    return c.k.aligned(16, 2);
}

template <int DT, int D>
void nc_mfma_launch(const NcCall& c, dim3 grid, hipStream_t st) {
    using T = typename Elem<DT>::T;
    KVP_LAUNCH("ncattn_mfma", st,
               ncattn_mfma_kernel<DT, D><<<grid, NC_THREADS, 0, st>>>((const T*)c.q.p, c.q.sb, (int)c.q.sh, (int)c.q.ss, (const T*)c.r.cosp, (const T*)c.r.sinp, c.r.sb,
                                                                     (int)c.r.sw, (const T*)c.k.p, c.k.sb, c.k.sh, (int)c.k.ss, (const T*)c.v.p, c.v.sb, c.v.sh,
                                                                     (int)c.v.ss, c.Hkv, c.G, c.S, c.C, c.tmp));
}

template <int DT>
int nc_run(const NcCall& c, bool mfma, dim3 grid, hipStream_t st) {
    using T = typename Elem<DT>::T;
    if constexpr (DT != KVP_F32) {
        if (mfma) {
            switch (c.D) {
                case 64: nc_mfma_launch<DT, 64>(c, grid, st); break;
                case 96: nc_mfma_launch<DT, 96>(c, grid, st); break;
                case 128: nc_mfma_launch<DT, 128>(c, grid, st); break;
                default: nc_mfma_launch<DT, 256>(c, grid, st); break;
            }
            KVP_CHECK_LAUNCH("ncattn_mfma_kernel");
            return KVP_OK;
        }
    }
    KVP_LAUNCH("ncattn_generic", st,
               ncattn_generic_kernel<DT><<<grid, GEN_THREADS, c.D * sizeof(float), st>>>((const T*)c.q.p, c.q.sb, c.q.sh, c.q.ss, (const T*)c.r.cosp, (const T*)c.r.sinp,
                                                                                         c.r.sb, c.r.sw, (const T*)c.k.p, c.k.sb, c.k.sh, c.k.ss, (const T*)c.v.p,
                                                                                         c.v.sb, c.v.sh, c.v.ss, c.Hkv, c.G, c.S, c.C, c.D, c.tmp));
    KVP_CHECK_LAUNCH("ncattn_generic_kernel");
    return KVP_OK;
}

// leverage workspace
struct LvWs {
    int nb, nb2;
    float *mpart, *gpart;
    double *A, *Y;
    float* minv;
    int* status;
    float* raw;
    ZsWs zs;
    size_t total;
};
LvWs lv_ws(void* ws, int64_t B, int64_t H, int64_t S, int64_t D, int64_t ks) {
    LvWs w;
    const int64_t BH = B * H;
    w.nb = (int)std::max<int64_t>(1, std::min<int64_t>((S + 1023) / 1024, 64));
    const int64_t ntiles = (S + LV_TILE - 1) / LV_TILE;
    const int64_t budget = (int64_t)8 << 20;   // partial Gram matrices: at most ~8 MiB (or one per head)
    w.nb2 = (int)std::max<int64_t>(1, std::min<int64_t>({(ntiles + 7) / 8, (int64_t)64, budget / std::max<int64_t>(1, BH * ks * ks * 4)}));
    KvpArena ar(ws);
    w.mpart = ar.take<float>((size_t)BH * w.nb * D);
    w.gpart = ar.take<float>((size_t)BH * w.nb2 * ks * ks);
    w.A = ar.take<double>((size_t)BH * ks * ks);
    w.Y = ar.take<double>((size_t)BH * ks * ks);
    w.minv = ar.take<float>((size_t)BH * ks * ks);
    w.status = ar.take<int>((size_t)BH);
    w.raw = ar.take<float>((size_t)BH * S);
    w.zs = zs_take(ar);
    w.total = ar.bytes();
    return w;
}

// phi [B,H,D,ks]: the sketch, element strides of its three outer dims in p.sb, p.sh, p.ss
template <int DT>
void lv_run(const LvWs& w, hipStream_t st, KvpRows k, KvpRows p, int B, int H, int S, int D, int ks, float* raw) {
    using T = typename Elem<DT>::T;
    KVP_LAUNCH("lv_mean", st, lv_mean_kernel<DT><<<dim3(w.nb, B * H), LV_THREADS, 0, st>>>((const T*)k.p, k.sb, k.sh, k.ss, H, S, D, w.nb, w.mpart));
    // entries per thread of an RB-row block of G: RB * ks / 256 (<= 16), rounded up to the next instantiated count; as few row blocks as that allows
    // (every row block recomputes the sketch of its tokens)
    const int RB = std::max(1, std::min(ks, 16 * LV_THREADS / ks));
    const int ntiles = (S + LV_TILE - 1) / LV_TILE;
    const dim3 gg(w.nb2, B * H, (ks + RB - 1) / RB);
    const int nu = (RB * ks + LV_THREADS - 1) / LV_THREADS;
#define LV_GRAM(NU_)                                                                                                                     \
    KVP_LAUNCH("lv_gram", st, lv_gram_kernel<DT, NU_><<<gg, LV_THREADS, 0, st>>>((const T*)k.p, k.sb, k.sh, k.ss, (const T*)p.p, p.sb, p.sh, \
                                                                                p.ss, H, S, D, ks, w.nb, w.mpart, w.nb2, RB, w.gpart))
    if (nu <= 2) LV_GRAM(2);
    else if (nu <= 4) LV_GRAM(4);
    else if (nu <= 6) LV_GRAM(6);
    else if (nu <= 8) LV_GRAM(8);
    else if (nu <= 9) LV_GRAM(9);     // sketch 48: 48 x 48 entries
    else if (nu <= 12) LV_GRAM(12);
    else LV_GRAM(16);
#undef LV_GRAM
    KVP_LAUNCH("lv_chol", st, lv_chol_kernel<<<B * H, LV_THREADS, 0, st>>>(w.gpart, w.nb2, ks, w.A, w.Y, w.minv, w.status));
    KVP_LAUNCH("lv_score", st,
               lv_score_kernel<DT><<<dim3(ntiles, B * H), LV_THREADS, 0, st>>>((const T*)k.p, k.sb, k.sh, k.ss, (const T*)p.p, p.sb, p.sh, p.ss, H, S, D, ks, w.nb,
                                                                                w.mpart, w.minv, raw));
}

}  // namespace

// ================================================================================================================================
extern "C" size_t kvp_ncattn_workspace_bytes(int64_t B, int64_t Hkv, int64_t S) {
    if (B < 1 || Hkv < 1 || S < 1) return 0;
    return nc_ws(nullptr, B, Hkv, S).total;
}

extern "C" int kvp_ncattn_score(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_ss, const void* cos, const void* sin, int64_t cs_sb,
                                int64_t cs_ss, const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss, const void* v, int64_t v_sb,
                                int64_t v_sh, int64_t v_ss, int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t S, int64_t D,
                                int64_t chunk, float* raw, float* scores, void* ws, size_t ws_bytes, kvp_stream_t stream) {
    NcCall c{{q, q_sb, q_sh, q_ss}, {k, k_sb, k_sh, k_ss}, {v, v_sb, v_sh, v_ss}, {cos, sin, cs_sb, cs_ss}};
    KVP_CHECK_ARG(q && cos && sin && k && v && scores && ws, "kvp_ncattn_score: null pointer");
    KVP_CHECK_DTYPE("kvp_ncattn_score", dtype);
    KVP_CHECK_ARG(chunk >= 1, "kvp_ncattn_score: chunk_size must be positive (got %lld)", (long long)chunk);
    KVP_CHECK_ARG(B >= 1 && Hkv >= 1 && Hq >= Hkv && Hq % Hkv == 0, "kvp_ncattn_score: bad shape (Hq %% Hkv != 0: Hq=%lld Hkv=%lld)",
                  (long long)Hq, (long long)Hkv);
    KVP_CHECK_ARG(S >= 1 && S < (1LL << 31) && D >= 2 && D % 2 == 0 && D <= 4096, "kvp_ncattn_score: bad shape (S=%lld D=%lld)", (long long)S,
                  (long long)D);
    KVP_CHECK_ARG(chunk <= (1LL << 30) && Hkv <= 65535 && B <= 65535, "kvp_ncattn_score: bad shape");
    const NcWs w = nc_ws(ws, B, Hkv, S);
    KVP_CHECK_ARG(ws_bytes >= w.total, "kvp_ncattn_score: workspace too small (%zu < %zu)", ws_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    const int64_t nchunks = (S + chunk - 1) / chunk;
    KVP_CHECK_ARG(nchunks <= 0x7fffffff, "kvp_ncattn_score: bad shape");
    c.Hkv = (int)Hkv; c.G = (int)(Hq / Hkv); c.S = (int)S; c.C = (int)chunk; c.D = (int)D; c.tmp = w.tmp;
    const bool mfma = nc_mfma_ok(c, dtype);
    const dim3 grid((unsigned)nchunks, (unsigned)Hkv, (unsigned)B);
    int rc;
    KVP_DISPATCH_DTYPE(dtype, rc = nc_run<DT>(c, mfma, grid, st));   // (mfma is false for float32: nc_mfma_ok)
    if (rc != KVP_OK) return rc;
    return zscore_launch(w.tmp, raw ? raw : w.raw, B * Hkv * S, S, 1, scores, w.zs, st);
}

extern "C" size_t kvp_leverage_workspace_bytes(int64_t B, int64_t H, int64_t S, int64_t D, int64_t sketch) {
    if (B < 1 || H < 1 || S < 1 || D < 1 || sketch < 1) return 0;
    return lv_ws(nullptr, B, H, S, D, sketch).total;
}

extern "C" int kvp_leverage_score(const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss, const void* phi, int64_t p_sb, int64_t p_sh,
                                  int64_t p_sd, int dtype, int64_t B, int64_t H, int64_t S, int64_t D, int64_t sketch, float* raw,
                                  float* scores, void* ws, size_t ws_bytes, kvp_stream_t stream) {
    KVP_CHECK_ARG(k && phi && scores && ws, "kvp_leverage_score: null pointer");
    KVP_CHECK_DTYPE("kvp_leverage_score", dtype);
    KVP_CHECK_ARG(sketch >= 1 && sketch <= 256, "kvp_leverage_score: sketch_dimension must be in [1, 256] (got %lld)", (long long)sketch);
    KVP_CHECK_ARG(B >= 1 && H >= 1 && B * H <= 65535 && S >= 1 && S < (1LL << 31) && D >= 1 && D <= 256,
                  "kvp_leverage_score: bad shape (B=%lld H=%lld S=%lld D=%lld; D <= 256)", (long long)B, (long long)H, (long long)S, (long long)D);
    const LvWs w = lv_ws(ws, B, H, S, D, sketch);
    KVP_CHECK_ARG(ws_bytes >= w.total, "kvp_leverage_score: workspace too small (%zu < %zu)", ws_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    float* rawp = raw ? raw : w.raw;
    KVP_DISPATCH_DTYPE(dtype, lv_run<DT>(w, st, {k, k_sb, k_sh, k_ss}, {phi, p_sb, p_sh, p_sd}, (int)B, (int)H, (int)S, (int)D, (int)sketch, rawp));
    KVP_CHECK_LAUNCH("kvp_leverage_score");
    return zscore_launch(rawp, rawp, B * H * S, S, 0, scores, w.zs, st);
}

extern "C" int kvp_leverage_status(const void* ws, int64_t B, int64_t H, int64_t S, int64_t D, int64_t sketch, kvp_stream_t stream) {
    KVP_CHECK_ARG(ws, "kvp_leverage_status: null pointer");
    KVP_CHECK_ARG(B >= 1 && H >= 1 && B * H <= 65535 && sketch >= 1 && sketch <= 256, "kvp_leverage_status: bad shape");
    const LvWs w = lv_ws(const_cast<void*>(ws), B, H, S, D, sketch);
    std::vector<int> st((size_t)(B * H));
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(st.data(), w.status, st.size() * sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        kvp_set_error("kvp_leverage_status: %s", hipGetErrorString(e));
        return KVP_EHIP;
    }
    for (size_t i = 0; i < st.size(); ++i)
        if (st[i] != 0) {
            kvp_set_error("kvp_leverage_score: Cholesky failed after 5 tries (b=%lld, head=%lld)", (long long)(i / H), (long long)(i % H));
            return KVP_ENUMERIC;
        }
    return KVP_OK;
}

extern "C" size_t kvp_compactor_combine_workspace_bytes(void) { return ZS_BLOCKS * sizeof(float); }

extern "C" int kvp_compactor_combine(const float* z_lev, const float* z_attn, int64_t B, int64_t H, int64_t S_inner, int64_t sink_start,
                                     int64_t sink_end, float blending, float* scores, void* ws, size_t ws_bytes, kvp_stream_t stream) {
    KVP_CHECK_ARG(z_lev && z_attn && scores && ws, "kvp_compactor_combine: null pointer");
    KVP_CHECK_ARG(B >= 1 && H >= 1 && S_inner >= 1 && sink_start >= 0 && sink_end >= 0, "kvp_compactor_combine: bad shape");
    KVP_CHECK_ARG(ws_bytes >= ZS_BLOCKS * sizeof(float), "kvp_compactor_combine: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    float* pmax = (float*)ws;
    const int64_t R = B * H;
    KVP_LAUNCH("cpt_blend", st, cpt_blend_kernel<<<ZS_BLOCKS, GEN_THREADS, 0, st>>>(z_lev, z_attn, R, S_inner, sink_start, sink_end, blending,
                                                                                    scores, pmax));
    KVP_CHECK_LAUNCH("cpt_blend_kernel");
    const int64_t ns = R * (sink_start + sink_end);
    if (ns > 0) {
        const unsigned nb = (unsigned)std::min<int64_t>((ns + GEN_THREADS - 1) / GEN_THREADS, 1024);
        KVP_LAUNCH("cpt_pad", st, cpt_pad_kernel<<<nb, GEN_THREADS, 0, st>>>(R, S_inner, sink_start, sink_end, pmax, scores));
        KVP_CHECK_LAUNCH("cpt_pad_kernel");
    }
    return KVP_OK;
}
