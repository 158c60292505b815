// CAMPress (kvpress/presses/cam_press.py; include/kvpress_hip.h: kvp_cam_*): cache merging while the model decodes.
//   (a) kvp_cam_attn_accumulate (:258-283, :326-361): the attention row of the newest token over all S keys, its mean over the G query
//       heads of a kv head, added in place to the layer's running sum.  Two launches: pass 1 walks the keys once -- a workgroup per
//       (b, kv head, chunk of keys), the RoPE'd queries of the group in registers, K straight from memory in 16-byte pieces -- and
//       leaves the logits (log2 units, float32 [B*Hq, S]) and one (max, sum) partial per chunk and query head (softmax_stats.h); pass 2
//       folds the partials of a row in chunk order and writes running[s] = (s < S_prev ? running[s] : 0) + mean_g 2^(L - norm_g).
//       kvp_cam_attn_accumulate_row is pass 2 alone on a given attention row.
//   (b) kvp_cam_merge_plan (:159-183): per merge candidate its window start in the kept list, and per kv head the merge probability.
//   (c) kvp_cam_merge_prune (:188-213): K', A' gathered at the kept positions, V' = the kept value plus the masked candidates whose window
//       covers the row -- a contiguous range of candidates (the starts are non-decreasing), found by two binary searches, summed in
//       ascending candidate order.  The inputs are never written.
// No atomics anywhere: every result is bit-identical from run to run.
#include <math.h>

#include "softmax_stats.h"

namespace {

constexpr int CT = 256;            // threads of every kernel here
constexpr int CAM_MAX_G = 16;      // query heads per kv head
constexpr int CAM_MAX_D = 256;
constexpr int CAM_MAX_CHUNKS = 256;

// keys per pass-1 workgroup: about 1024 workgroups over all rows, chunks of whole 64-key groups, at most CAM_MAX_CHUNKS per row
int64_t cam_chunk(int64_t R, int64_t S) {
    int64_t c = (S * R + 1023) / 1024;
    c = std::max<int64_t>(c, (S + CAM_MAX_CHUNKS - 1) / CAM_MAX_CHUNKS);
    return std::max<int64_t>(64, (c + 63) / 64 * 64);
}

struct CamWs {
    int64_t chunk, nchunk;
    float *logits, *pm, *pz;   // [B*Hq][S], [B*Hq][nchunk] twice
    size_t total;
};
CamWs cam_ws(void* ws, int64_t B, int64_t Hq, int64_t Hkv, int64_t S) {
    CamWs L;
    L.chunk = cam_chunk(B * Hkv, S);
    L.nchunk = (S + L.chunk - 1) / L.chunk;
    KvpArena ar(ws);
    L.logits = ar.take<float>((size_t)B * Hq * S);
    L.pm = ar.take<float>((size_t)B * Hq * L.nchunk);
    L.pz = ar.take<float>((size_t)B * Hq * L.nchunk);
    L.total = ar.bytes();
    return L;
}

struct CamAttnArgs {
    const void *q, *cosp, *sinp, *k;
    int64_t q_sb, q_sh, cs_sb, k_sb, k_sh, k_ss;
    int Hq, G, D;
    int gsub, nsub;   // pass 1: the query heads of a kv head are walked nsub workgroups of gsub heads each (G > 8: two halves)
    int64_t S, chunk, nchunk;
    float scale;   // log2(e) / sqrt(D)
    float *logits, *pm, *pz;
};

// q_rot = q * cos + rotate_half(q) * sin of the query heads h0 .. h0 + n, rounded as torch does in the model dtype (rope_elem), as floats [n][D]
template <int DT>
__device__ __forceinline__ void cam_rope_group(const CamAttnArgs& a, int64_t b, int h0, int n, float* qs) {
    using T = typename Elem<DT>::T;
    const int half = a.D / 2;
    const T* cr = (const T*)a.cosp + b * a.cs_sb;
    const T* sr = (const T*)a.sinp + b * a.cs_sb;
    for (int i = threadIdx.x; i < n * half; i += CT) {
        const int g = i / half, d = i % half;
        const T* qr = (const T*)a.q + b * a.q_sb + (int64_t)(h0 + g) * a.q_sh;
        const float q0 = Elem<DT>::ld(qr + d), q1 = Elem<DT>::ld(qr + d + half);
        qs[g * a.D + d] = rope_elem<DT>(q0, Elem<DT>::ld(cr + d), -q1, Elem<DT>::ld(sr + d));
        qs[g * a.D + d + half] = rope_elem<DT>(q1, Elem<DT>::ld(cr + d + half), q0, Elem<DT>::ld(sr + d + half));
    }
}

// the workgroup's (m, z) of query head g: the waves' partials in wave order (thread 0 writes)
__device__ __forceinline__ void cam_store_partial(float m, float z, float* red, float* pm, float* pz, int64_t slot) {
    wave_softmax_merge(m, z);
    __syncthreads();   // red is reused from head to head
    if ((threadIdx.x & 63) == 0) {
        red[2 * (threadIdx.x >> 6)] = m;
        red[2 * (threadIdx.x >> 6) + 1] = z;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float mm = red[0], zz = red[1];
        for (int w = 1; w < CT / 64; ++w) softmax_merge(mm, zz, red[2 * w], red[2 * w + 1]);
        pm[slot] = mm;
        pz[slot] = zz;
    }
}

// ---- (a) pass 1, vector path: rows of whole 16-byte pieces, 16-byte aligned.  LPK (a power of two >= the pieces of a row) lanes share a
// key: lane c of them owns piece c of the key AND of every query of the group (registers), the dot products meet by a butterfly over
// the LPK lanes; query head g is then kept (logit, running max and sum) by lane g % LPK.  GP <= 8 = the heads of a workgroup rounded up to a
// power of two: a group of 9 .. 16 query heads is walked by two workgroups (16 heads in one kept 16 loop-invariant lane masks in scalar
// registers and spilled them).
template <int DT, int GP>
__global__ __launch_bounds__(CT) void cam_logits_vec_kernel(CamAttnArgs a, int LPK) {
    using T = typename Elem<DT>::T;
    constexpr int PER = Elem<DT>::PER16;
    constexpr int U = GP <= 2 ? 4 : 2;   // keys in flight per lane group
    __shared__ float qs[8 * CAM_MAX_D];
    __shared__ float red[2 * (CT / 64)];
    const int64_t b = blockIdx.z;
    const int hkv = blockIdx.y / a.nsub;
    const int g0 = (blockIdx.y % a.nsub) * a.gsub, gn = min(a.gsub, a.G - g0);   // this workgroup's query heads of the group
    const int h0 = hkv * a.G + g0;
    cam_rope_group<DT>(a, b, h0, gn, qs);
    __syncthreads();
    const int c = threadIdx.x & (LPK - 1);
    const bool live = c * PER < a.D;
    float qr[GP][PER];
#pragma unroll
    for (int g = 0; g < GP; ++g)
#pragma unroll
        for (int e = 0; e < PER; ++e) qr[g][e] = (live && g < gn) ? qs[g * a.D + c * PER + e] : 0.f;
    float m[GP], z[GP];
#pragma unroll
    for (int g = 0; g < GP; ++g) {
        m[g] = KVP_NEG_INF;
        z[g] = 0.f;
    }
    const int kpi = CT / LPK;   // keys per sweep of the workgroup
    const int64_t s0 = (int64_t)blockIdx.x * a.chunk, s1 = min(a.S, s0 + a.chunk);
    const T* kb = (const T*)a.k + b * a.k_sb + (int64_t)hkv * a.k_sh + c * PER;
    float* lrow = a.logits + (b * a.Hq + h0) * a.S;
    for (int64_t sb = s0 + threadIdx.x / LPK; sb < s1; sb += (int64_t)U * kpi) {
        uint4 kv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t s = sb + (int64_t)u * kpi;
            kv[u] = (live && s < s1) ? ld16<false>(kb + s * a.k_ss) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t s = sb + (int64_t)u * kpi;   // (the lanes of a key agree on s < s1: the butterfly below stays inside them)
            float f[PER];
            unpack16<DT>(kv[u], f);
            float acc[GP];
#pragma unroll
            for (int g = 0; g < GP; ++g) {
                acc[g] = 0.f;
#pragma unroll
                for (int e = 0; e < PER; ++e) acc[g] = fmaf(f[e], qr[g][e], acc[g]);
            }
            for (int o = LPK >> 1; o > 0; o >>= 1) {
#pragma unroll
                for (int g = 0; g < GP; ++g) acc[g] += __shfl_xor(acc[g], o);
            }
            if (s < s1) {
#pragma unroll
                for (int g = 0; g < GP; ++g) {
                    if (g < gn && (g & (LPK - 1)) == c) {
                        const float l2 = acc[g] * a.scale;
                        lrow[(int64_t)g * a.S + s] = l2;
                        softmax_merge(m[g], z[g], l2, 1.f);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int g = 0; g < GP; ++g) {
        if (g < gn) cam_store_partial(m[g], z[g], red, a.pm, a.pz, (b * a.Hq + h0 + g) * a.nchunk + blockIdx.x);
    }
}

// ---- (a) pass 1, generic path: any D <= 256, any alignment (the tiny test models: D = 6).  A thread per key, a sweep per query head.
template <int DT>
__global__ __launch_bounds__(CT) void cam_logits_generic_kernel(CamAttnArgs a) {
    using T = typename Elem<DT>::T;
    __shared__ float qs[CAM_MAX_G * CAM_MAX_D];
    __shared__ float red[2 * (CT / 64)];
    const int64_t b = blockIdx.z;
    const int hkv = blockIdx.y;
    cam_rope_group<DT>(a, b, hkv * a.G, a.G, qs);
    __syncthreads();
    const int64_t s0 = (int64_t)blockIdx.x * a.chunk, s1 = min(a.S, s0 + a.chunk);
    const T* kb = (const T*)a.k + b * a.k_sb + (int64_t)hkv * a.k_sh;
    for (int g = 0; g < a.G; ++g) {
        float m = KVP_NEG_INF, z = 0.f;
        float* lrow = a.logits + (b * a.Hq + (int64_t)hkv * a.G + g) * a.S;
        for (int64_t s = s0 + threadIdx.x; s < s1; s += CT) {
            const T* kr = kb + s * a.k_ss;
            float acc = 0.f;
            for (int d = 0; d < a.D; ++d) acc = fmaf(Elem<DT>::ld(kr + d), qs[g * a.D + d], acc);
            const float l2 = acc * a.scale;
            lrow[s] = l2;
            softmax_merge(m, z, l2, 1.f);
        }
        cam_store_partial(m, z, red, a.pm, a.pz, (b * a.Hq + (int64_t)hkv * a.G + g) * a.nchunk + blockIdx.x);
    }
}

// ---- (a) pass 2: running[s] = (s < S_prev ? running[s] : 0) + mean over the group of 2^(L - norm); norm from the partials in chunk order
__global__ __launch_bounds__(CT) void cam_accumulate_kernel(const float* __restrict__ logits, const float* __restrict__ pm,
                                                            const float* __restrict__ pz, int Hq, int G, int64_t S, int64_t nchunk,
                                                            float* __restrict__ running, int64_t r_sb, int64_t r_sh, int64_t s_prev) {
    __shared__ float norm[CAM_MAX_G];
    const int64_t b = blockIdx.z;
    const int hkv = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int64_t row0 = b * Hq + (int64_t)hkv * G;
    for (int g = threadIdx.x >> 6; g < G; g += CT / 64) {
        float m = KVP_NEG_INF, z = 0.f;
        for (int64_t j = lane; j < nchunk; j += 64) softmax_merge(m, z, pm[(row0 + g) * nchunk + j], pz[(row0 + g) * nchunk + j]);
        wave_softmax_merge(m, z);
        if (lane == 0) norm[g] = m + log2f(z);
    }
    __syncthreads();
    const int64_t s = (int64_t)blockIdx.x * CT + threadIdx.x;
    if (s >= S) return;
    float sum = 0.f;
    for (int g = 0; g < G; ++g) sum += exp2f(logits[(row0 + g) * S + s] - norm[g]);
    float* r = running + b * r_sb + (int64_t)hkv * r_sh + s;
    *r = (s < s_prev ? *r : 0.f) + sum / (float)G;
}

// the same from the attention row the layer returned (cam_press.py:259-263): attn [B,Hq,S]
template <int DT>
__global__ __launch_bounds__(CT) void cam_accumulate_row_kernel(const typename Elem<DT>::T* __restrict__ attn, int64_t a_sb, int64_t a_sh, int G,
                                                                int64_t S, float* __restrict__ running, int64_t r_sb, int64_t r_sh,
                                                                int64_t s_prev) {
    const int64_t b = blockIdx.z;
    const int hkv = blockIdx.y;
    const int64_t s = (int64_t)blockIdx.x * CT + threadIdx.x;
    if (s >= S) return;
    float sum = 0.f;
    for (int g = 0; g < G; ++g) sum += Elem<DT>::ld(attn + b * a_sb + ((int64_t)hkv * G + g) * a_sh + s);
    float* r = running + b * r_sb + (int64_t)hkv * r_sh + s;
    *r = (s < s_prev ? *r : 0.f) + sum / (float)G;
}

// number of entries of the ascending list x[0..n) that are <= v (upper bound) / < v (lower bound)
__device__ __forceinline__ int cam_count_le(const int32_t* __restrict__ x, int n, int v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (x[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ int cam_count_lt(const int32_t* __restrict__ x, int n, int v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (x[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- (b) plan: a thread per (entry of sel, kv head, batch) ---------------------------------------------------------------------------
// sel is either the M candidates themselves (N == M) or the ascending superset kept + candidates (N == T + M: two position-order
// selects, top T inside top T + M); then entry j with c kept positions below it is candidate j - c, and the same search gives its start.
__global__ __launch_bounds__(CT) void cam_plan_kernel(const int32_t* __restrict__ kept, const int32_t* __restrict__ sel, int N,
                                                      const float* __restrict__ attn, int64_t a_sb, int64_t a_sh, int H, int64_t S, int T,
                                                      int M, int budget_max, int32_t* __restrict__ cand, int32_t* __restrict__ start,
                                                      float* __restrict__ prob) {
    const int64_t b = blockIdx.z;
    const int h = blockIdx.y;
    const int j = blockIdx.x * CT + threadIdx.x;
    if (j >= N) return;
    const int32_t* kp = kept + b * T;
    const float* ar = attn + b * a_sb + (int64_t)h * a_sh;
    const int p = sel[b * N + j];
    const int below = cam_count_lt(kp, T, p);
    int i = j, st = below;
    if (below < T && kp[below] == p) {
        if (N != M) return;                             // a kept position of the superset
        st = below + 1;                                 // (a candidate that is also kept: searchsorted(right=True) counts it, :159)
    }
    if (N != M) i = j - below;
    if (i < 0 || i >= M) return;                        // the superset does not hold the kept list
    const int budget = min(budget_max, T - st);         // :164-169
    float sum = 0.f;
    for (int w = 0; w < budget; ++w) {
        const int t = kp[st + w];
        if (t >= 0 && t < S) sum += ar[t];
    }
    const float mean = sum / (float)max(budget, 1);     // :176
    float x = (p >= 0 && p < S) ? ar[p] / mean : 0.f;   // :179-183
    if (isnan(x)) x = 0.f;
    if (isinf(x)) x = 1.f;
    x = fminf(fmaxf(x, 0.f), 1.f);
    prob[(b * H + h) * (int64_t)M + i] = x;
    if (h == 0) {
        start[b * M + i] = st;
        if (cand) cand[b * M + i] = p;
    }
}

__device__ __forceinline__ void cam_all_ones(float* p) { *p = __uint_as_float(0xFFFFFFFFu); }
__device__ __forceinline__ void cam_all_ones(uint16_t* p) { *p = 0xFFFFu; }
__device__ __forceinline__ void cam_all_ones(_Float16* p) { *reinterpret_cast<uint16_t*>(p) = 0xFFFFu; }

// ---- (c) merge and prune: a wave per row (b, h, t) of the outputs --------------------------------------------------------------------
// V'[t] = V[kept[t]] + sum over the candidates i with start_i <= t < start_i + m of mask_i / budget_i * V[cand_i] (t < T makes the
// window's clip at T automatic), in ascending i; float32 with the rounding error of every product and sum carried along (a second
// float per element), one rounding to the dtype.  The values are read and written an element per lane (lane l owns elements l, l + 64, ..:
// the sum needs them as floats), K' moves in 16-byte pieces where the rows allow it.  An invalid kept position gives a row of all-ones bit patterns, as kvp_gather_kv does.
template <int DT>
__global__ __launch_bounds__(CT) void cam_prune_kernel(const typename Elem<DT>::T* __restrict__ k, int64_t k_sb, int64_t k_sh, int64_t k_ss,
                                                       const typename Elem<DT>::T* __restrict__ v, int64_t v_sb, int64_t v_sh, int64_t v_ss,
                                                       const float* __restrict__ attn, int64_t a_sb, int64_t a_sh,
                                                       const int32_t* __restrict__ kept, const int32_t* __restrict__ cand,
                                                       const int32_t* __restrict__ start, const float* __restrict__ mask, int H, int64_t S, int T,
                                                       int M, int D, int budget_max, bool kvec, typename Elem<DT>::T* __restrict__ ko,
                                                       typename Elem<DT>::T* __restrict__ vo, float* __restrict__ ao) {
    using T_ = typename Elem<DT>::T;
    const int64_t b = blockIdx.z;
    const int h = blockIdx.y;
    const int t = blockIdx.x * (CT / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= T) return;
    const int64_t r = b * H + h;
    const int p = kept[b * T + t];
    T_* korow = ko + (r * T + t) * D;
    T_* vorow = vo + (r * T + t) * D;
    if (p < 0 || p >= S) {
        for (int d = lane; d < D; d += 64) {
            cam_all_ones(korow + d);
            cam_all_ones(vorow + d);
        }
        if (lane == 0) ao[r * T + t] = __uint_as_float(0xFFFFFFFFu);
        return;
    }
    const T_* krow = k + b * k_sb + (int64_t)h * k_sh + (int64_t)p * k_ss;
    const T_* vb = v + b * v_sb + (int64_t)h * v_sh;
    float acc[4], err[4];
    bool merged = false;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int d = lane + 64 * q;
        if (!kvec && d < D) korow[d] = krow[d];
        acc[q] = d < D ? Elem<DT>::ld(vb + (int64_t)p * v_ss + d) : 0.f;
        err[q] = 0.f;
    }
    if (kvec && lane * Elem<DT>::PER16 < D) {   // aligned key rows of whole 16-byte pieces (at most 64 of them): one piece per lane
        st16<false>(korow + lane * Elem<DT>::PER16, ld16<false>(krow + lane * Elem<DT>::PER16));
    }
    if (lane == 0) ao[r * T + t] = attn[b * a_sb + (int64_t)h * a_sh + p];
    const int32_t* sp = start + b * M;
    const int lo = cam_count_lt(sp, M, t - budget_max + 1), hi = cam_count_le(sp, M, t);
    for (int i = lo; i < hi; ++i) {
        const float mk = mask[r * M + i];
        const int pc = cand[b * M + i];
        const int bud = min(budget_max, T - sp[i]);
        if (mk == 0.f || pc < 0 || pc >= S || bud < 1) continue;   // :192-193: a masked-out candidate adds nothing
        const float w = mk / (float)bud;
        const T_* vr = vb + (int64_t)pc * v_ss;
        merged = true;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int d = lane + 64 * q;
            if (d < D) {
                const float x = Elem<DT>::ld(vr + d);
                const float pr = __fmul_rn(w, x);
                const float pe = fmaf(w, x, -pr);                    // the product's rounding error
                const float s = __fadd_rn(acc[q], pr);
                const float bb = __fsub_rn(s, acc[q]);
                const float se = __fadd_rn(__fsub_rn(acc[q], __fsub_rn(s, bb)), __fsub_rn(pr, bb));   // the sum's
                acc[q] = s;
                err[q] = __fadd_rn(err[q], __fadd_rn(se, pe));
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int d = lane + 64 * q;
        if (d < D) {
            if (merged) vorow[d] = to_dt_acc<DT>(__fadd_rn(acc[q], err[q]));
            else vorow[d] = vb[(int64_t)p * v_ss + d];               // no contributor: the stored bits
        }
    }
}

bool cam_vec_ok(int dtype, int64_t D, KvpRows k) {
    const int per = 16 / kvp_elem_size(dtype);
    return D % per == 0 && D / per <= 64 && k.aligned(16, kvp_elem_size(dtype));
}

template <int DT>
int cam_attn_run(const CamAttnArgs& a, int64_t B, int64_t Hkv, bool vec, hipStream_t st) {
    if (vec) {
        const dim3 grid((unsigned)a.nchunk, (unsigned)(Hkv * a.nsub), (unsigned)B);
        const int pieces = a.D / Elem<DT>::PER16;
        int lpk = 1;
        while (lpk < pieces) lpk <<= 1;
        if (a.gsub <= 1) KVP_LAUNCH("cam_logits", st, cam_logits_vec_kernel<DT, 1><<<grid, CT, 0, st>>>(a, lpk));
        else if (a.gsub <= 2) KVP_LAUNCH("cam_logits", st, cam_logits_vec_kernel<DT, 2><<<grid, CT, 0, st>>>(a, lpk));
        else if (a.gsub <= 4) KVP_LAUNCH("cam_logits", st, cam_logits_vec_kernel<DT, 4><<<grid, CT, 0, st>>>(a, lpk));
        else KVP_LAUNCH("cam_logits", st, cam_logits_vec_kernel<DT, 8><<<grid, CT, 0, st>>>(a, lpk));
    } else {
        const dim3 grid((unsigned)a.nchunk, (unsigned)Hkv, (unsigned)B);
        KVP_LAUNCH("cam_logits_generic", st, cam_logits_generic_kernel<DT><<<grid, CT, 0, st>>>(a));
    }
    KVP_CHECK_LAUNCH("kvp_cam_attn_accumulate (logits)");
    return KVP_OK;
}

bool cam_running_ok(int64_t B, int64_t Hkv, int64_t S, int64_t r_sb, int64_t r_sh, int64_t cap, int64_t s_prev) {
    return cap >= S && s_prev >= 0 && s_prev <= S && (Hkv == 1 || r_sh >= cap) && (B == 1 || r_sb >= r_sh * (Hkv - 1) + cap);
}

}  // namespace

// ================================================================================================================================
extern "C" size_t kvp_cam_attn_workspace_bytes(int64_t B, int64_t Hq, int64_t Hkv, int64_t S) {
    if (B < 1 || Hq < 1 || Hkv < 1 || S < 1 || Hq % Hkv != 0) return 0;
    return cam_ws(nullptr, B, Hq, Hkv, S).total;
}

extern "C" int kvp_cam_attn_accumulate(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_sw, const void* cosp, const void* sinp,
                                       int64_t cs_sb, int64_t cs_sw, const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss, int dtype,
                                       int64_t B, int64_t Hq, int64_t Hkv, int64_t S, int64_t D, float* running, int64_t r_sb, int64_t r_sh,
                                       int64_t cap, int64_t S_prev, void* ws, size_t ws_bytes, kvp_stream_t stream) {
    (void)q_sw;   // one query row
    (void)cs_sw;
    const KvpRows kr{k, k_sb, k_sh, k_ss};
    KVP_CHECK_DTYPE("kvp_cam_attn_accumulate", dtype);
    KVP_CHECK_ARG(B >= 1 && Hq >= 1 && Hkv >= 1 && S >= 1 && D >= 2 && Hq % Hkv == 0, "kvp_cam_attn_accumulate: bad shape");
    KVP_CHECK_ARG(D % 2 == 0 && D <= CAM_MAX_D, "kvp_cam_attn_accumulate: head size %lld is odd or > 256", (long long)D);
    KVP_CHECK_ARG(Hq / Hkv <= CAM_MAX_G, "kvp_cam_attn_accumulate: more than 16 query heads per kv head (%lld)", (long long)(Hq / Hkv));
    KVP_CHECK_ARG(S < ((int64_t)1 << 31) && B < 65536 && Hkv < 32768, "kvp_cam_attn_accumulate: bad shape (S, B or Hkv too large)");
    KVP_CHECK_ARG(cam_running_ok(B, Hkv, S, r_sb, r_sh, cap, S_prev), "kvp_cam_attn_accumulate: bad running sum (cap < S, S_prev outside [0, S] or overlapping rows)");
    KVP_CHECK_ARG(q && cosp && sinp && k && running, "kvp_cam_attn_accumulate: null pointer");
    const CamWs L = cam_ws(ws, B, Hq, Hkv, S);
    if (int rc = kvp_check_workspace("kvp_cam_attn_accumulate", ws, ws_bytes, L.total)) return rc;
    hipStream_t st = (hipStream_t)stream;
    CamAttnArgs a;
    a.q = q; a.cosp = cosp; a.sinp = sinp; a.k = k;
    a.q_sb = q_sb; a.q_sh = q_sh; a.cs_sb = cs_sb; a.k_sb = k_sb; a.k_sh = k_sh; a.k_ss = k_ss;
    a.Hq = (int)Hq; a.G = (int)(Hq / Hkv); a.D = (int)D;
    a.nsub = a.G > 8 ? 2 : 1;
    a.gsub = (a.G + a.nsub - 1) / a.nsub;
    a.S = S; a.chunk = L.chunk; a.nchunk = L.nchunk;
    a.scale = (float)(1.4426950408889634 / sqrt((double)D));
    a.logits = L.logits; a.pm = L.pm; a.pz = L.pz;
    const bool vec = cam_vec_ok(dtype, D, kr);
    KVP_DISPATCH_DTYPE(dtype, if (int rc = cam_attn_run<DT>(a, B, Hkv, vec, st)) return rc);
    const dim3 grid((unsigned)((S + CT - 1) / CT), (unsigned)Hkv, (unsigned)B);
    KVP_LAUNCH("cam_accumulate", st,
               cam_accumulate_kernel<<<grid, CT, 0, st>>>(a.logits, a.pm, a.pz, a.Hq, a.G, S, L.nchunk, running, r_sb, r_sh, S_prev));
    KVP_CHECK_LAUNCH("kvp_cam_attn_accumulate");
    return KVP_OK;
}

extern "C" int kvp_cam_attn_accumulate_row(const void* attn, int64_t a_sb, int64_t a_sh, int dtype, int64_t B, int64_t Hq, int64_t Hkv,
                                           int64_t S, float* running, int64_t r_sb, int64_t r_sh, int64_t cap, int64_t S_prev,
                                           kvp_stream_t stream) {
    KVP_CHECK_DTYPE("kvp_cam_attn_accumulate_row", dtype);
    KVP_CHECK_ARG(B >= 1 && Hq >= 1 && Hkv >= 1 && S >= 1 && Hq % Hkv == 0, "kvp_cam_attn_accumulate_row: bad shape");
    KVP_CHECK_ARG(S < ((int64_t)1 << 31) && B < 65536 && Hkv < 65536, "kvp_cam_attn_accumulate_row: bad shape (S, B or Hkv too large)");
    KVP_CHECK_ARG(cam_running_ok(B, Hkv, S, r_sb, r_sh, cap, S_prev), "kvp_cam_attn_accumulate_row: bad running sum (cap < S, S_prev outside [0, S] or overlapping rows)");
    KVP_CHECK_ARG(attn && running, "kvp_cam_attn_accumulate_row: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((S + CT - 1) / CT), (unsigned)Hkv, (unsigned)B);
    const int G = (int)(Hq / Hkv);
    KVP_DISPATCH_DTYPE(dtype, KVP_LAUNCH("cam_accumulate_row", st,
                                         cam_accumulate_row_kernel<DT><<<grid, CT, 0, st>>>((const typename Elem<DT>::T*)attn, a_sb, a_sh, G, S,
                                                                                            running, r_sb, r_sh, S_prev)));
    KVP_CHECK_LAUNCH("kvp_cam_attn_accumulate_row");
    return KVP_OK;
}

#define CAM_CHECK_PLAN_SHAPE(who)                                                                                                         \
    KVP_CHECK_ARG(B >= 1 && H >= 1 && S >= 1 && T >= 1 && M >= 0 && T <= S && M <= S - T, who ": bad shape (need 1 <= T <= S, 0 <= M <= S - T)"); \
    KVP_CHECK_ARG(S < ((int64_t)1 << 31) && B < 65536 && H < 65536, who ": bad shape (S, B or H too large)");                             \
    KVP_CHECK_ARG(merge_budget > 0, who ": merge_budget must be positive (%lld)", (long long)merge_budget)

extern "C" int kvp_cam_merge_plan(const int32_t* kept, const int32_t* sel, int64_t n_sel, const float* attn, int64_t a_sb, int64_t a_sh,
                                  int64_t B, int64_t H, int64_t S, int64_t T, int64_t M, int64_t merge_budget, int32_t* cand, int32_t* start,
                                  float* prob, kvp_stream_t stream) {
    CAM_CHECK_PLAN_SHAPE("kvp_cam_merge_plan");
    KVP_CHECK_ARG(n_sel == M || n_sel == T + M, "kvp_cam_merge_plan: n_sel must be M (the candidates) or T + M (kept and candidates)");
    if (M == 0) return KVP_OK;
    KVP_CHECK_ARG(kept && sel && attn && start && prob, "kvp_cam_merge_plan: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int bm = (int)std::min<int64_t>(merge_budget, T);
    KVP_LAUNCH("cam_plan", st,
               cam_plan_kernel<<<dim3((unsigned)((n_sel + CT - 1) / CT), (unsigned)H, (unsigned)B), CT, 0, st>>>(
                   kept, sel, (int)n_sel, attn, a_sb, a_sh, (int)H, S, (int)T, (int)M, bm, cand, start, prob));
    KVP_CHECK_LAUNCH("kvp_cam_merge_plan");
    return KVP_OK;
}

extern "C" int kvp_cam_merge_prune(const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss, const void* v, int64_t v_sb, int64_t v_sh,
                                   int64_t v_ss, const float* attn, int64_t a_sb, int64_t a_sh, const int32_t* kept, const int32_t* cand,
                                   const int32_t* start, const float* mask, int dtype, int64_t B, int64_t H, int64_t S, int64_t T, int64_t M,
                                   int64_t D, int64_t merge_budget, void* k_out, void* v_out, float* attn_out, kvp_stream_t stream) {
    KVP_CHECK_DTYPE("kvp_cam_merge_prune", dtype);
    CAM_CHECK_PLAN_SHAPE("kvp_cam_merge_prune");
    KVP_CHECK_ARG(D >= 1 && D <= CAM_MAX_D, "kvp_cam_merge_prune: head size %lld outside [1, 256]", (long long)D);
    KVP_CHECK_ARG(k && v && attn && kept && k_out && v_out && attn_out && (M == 0 || (cand && start && mask)), "kvp_cam_merge_prune: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int bm = (int)std::min<int64_t>(merge_budget, T);
    const dim3 grid((unsigned)((T + CT / 64 - 1) / (CT / 64)), (unsigned)H, (unsigned)B);
    const bool kvec = cam_vec_ok(dtype, D, {k, k_sb, k_sh, k_ss}) && !((uintptr_t)k_out & 15);
    KVP_DISPATCH_DTYPE(dtype, using T_ = typename Elem<DT>::T;
                       KVP_LAUNCH("cam_prune", st,
                                  cam_prune_kernel<DT><<<grid, CT, 0, st>>>((const T_*)k, k_sb, k_sh, k_ss, (const T_*)v, v_sb, v_sh, v_ss, attn, a_sb,
                                                                            a_sh, kept, cand, start, mask, (int)H, S, (int)T, (int)M, (int)D, bm, kvec,
                                                                            (T_*)k_out, (T_*)v_out, attn_out)));
    KVP_CHECK_LAUNCH("kvp_cam_merge_prune");
    return KVP_OK;
}
