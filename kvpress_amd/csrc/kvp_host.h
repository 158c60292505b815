// Host side of libkvpress_hip.so that more than one .hip uses: error / launch plumbing, the host-side views of the C ABI's flat
// arguments (KvpRows: a strided [B,H,S,D] tensor and its alignment test; KvpRope: the rotary tables), the workspace arena every
// layout is carved with (KvpArena), kvp_raise_dynamic_lds, and every launcher that one .hip defines and another calls (the families
// with a header of their own keep theirs: snapkv_internal.h, ea_internal.h, topk_internal.h).  An extern "C" entry builds its views
// once from its flat arguments; the flat lists come back only in a kernel launch expression.  Included by kvp_common.h.
// The library is compiled with -fvisibility=hidden: the extern "C" entries of
// include/*.h are exported (kvp_common.h), the KVP_INTERNAL_API functions below for csrc/contrib/*.hip, nothing else.
#pragma once

// needed by libkvpress_hip_contrib.so through KVP_CHECK_ARG / KVP_CHECK_LAUNCH / KVP_LAUNCH (tests/test_capi_symbols.py reads this list)
#define KVP_INTERNAL_API __attribute__((visibility("default")))

// ---- error reporting (thread-local last message; defined in capi.hip) ------------------------
KVP_INTERNAL_API void kvp_set_error(const char* fmt, ...);

#define KVP_CHECK_ARG(cond, ...)                 \
    do {                                         \
        if (!(cond)) {                           \
            kvp_set_error(__VA_ARGS__);          \
            return KVP_EINVAL;                   \
        }                                        \
    } while (0)

#define KVP_CHECK_DTYPE(who, dtype) KVP_CHECK_ARG(dtype == KVP_F32 || dtype == KVP_F16 || dtype == KVP_BF16, who ": bad dtype %d", dtype)

#define KVP_CHECK_LAUNCH(name)                                                     \
    do {                                                                           \
        hipError_t e__ = hipGetLastError();                                        \
        if (e__ != hipSuccess) {                                                   \
            kvp_set_error("%s: launch failed: %s", name, hipGetErrorString(e__));  \
            return KVP_EHIP;                                                       \
        }                                                                          \
    } while (0)

// KVP_OK, or KVP_EWORKSPACE with "<who>: workspace too small (have < need)"
inline int kvp_check_workspace(const char* who, const void* ws, size_t ws_bytes, size_t need) {
    if (ws && ws_bytes >= need) return KVP_OK;
    kvp_set_error("%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    return KVP_EWORKSPACE;
}

// ---- asynchronous failure reports (capi.hip) -------------------------------------------------------------------------------
// A kernel that detects at RUN time that its result is invalid (the cluster select when its workgroups never become co-resident,
// topk_cluster.hip) poisons its output AND stores a code into one process-wide, host-pinned status word; every entry point that
// produces or consumes a selection calls kvp_async_check() first and turns a pending report into KVP_EASYNC + kvp_last_error().
// The word holds (launch sequence number << 8) | code: all the stores of ONE failed launch make one report, however late the last of
// them lands (a repeat of a sequence number that was already reported is dropped).
uint32_t* kvp_async_flag();             // device-visible address of the status word (nullptr: pinned allocation failed -> poison only)
uint32_t kvp_async_next_seq();          // sequence number (1 .. 2^24 - 1, wrapping) for the next launch that may report
int kvp_async_check(const char* who);   // KVP_OK, or KVP_EASYNC exactly once per report

// ---- opt-in per-kernel timing (kvp_prof_* in include/kvpress_hip_lab.h; implemented in capi.hip) ----
KVP_INTERNAL_API bool kvp_prof_enabled();
KVP_INTERNAL_API void kvp_prof_begin(const char* name, hipStream_t stream);
KVP_INTERNAL_API void kvp_prof_end(hipStream_t stream);
// every kernel launch of the library goes through this macro
#define KVP_LAUNCH(name, stream, ...)                         \
    do {                                                      \
        const bool prof__ = kvp_prof_enabled();               \
        if (prof__) kvp_prof_begin(name, stream);             \
        __VA_ARGS__;                                          \
        if (prof__) kvp_prof_end(stream);                     \
    } while (0)

// `...` once, with DT a compile-time copy of `dtype` (which KVP_CHECK_DTYPE has validated)
#define KVP_DISPATCH_DTYPE(dtype, ...)                                       \
    switch (dtype) {                                                         \
        case KVP_F32: { constexpr int DT = KVP_F32; __VA_ARGS__; } break;    \
        case KVP_F16: { constexpr int DT = KVP_F16; __VA_ARGS__; } break;    \
        default: { constexpr int DT = KVP_BF16; __VA_ARGS__; } break;        \
    }

// tuning knobs read from the environment once (KVP_* variables; used for A/B runs on hardware)
int kvp_env_int(const char* name, int dflt);

static inline size_t kvp_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
static inline int kvp_elem_size(int dtype) { return dtype == KVP_F32 ? 4 : 2; }

// a [B, H, S, D] tensor as the C ABI passes it: base pointer + element strides of the three outer dims (rows contiguous)
struct KvpRows {
    const void* p;
    int64_t sb, sh, ss;
    // are the base pointer and the three strides multiples of `bytes` (a power of two), for elements of `es` bytes?
    bool aligned(size_t bytes, size_t es) const { return (((uintptr_t)p | (uintptr_t)sb * es | (uintptr_t)sh * es | (uintptr_t)ss * es) & (bytes - 1)) == 0; }
    // the view from row s on
    KvpRows from_row(int64_t s, size_t es) const { return {static_cast<const char*>(p) + s * ss * (int64_t)es, sb, sh, ss}; }
};
// the rotary tables cos, sin [1 or B, W, D]: element strides of the two outer dims
struct KvpRope {
    const void *cosp, *sinp;
    int64_t sb, sw;
    bool aligned(size_t bytes, size_t es) const { return (((uintptr_t)cosp | (uintptr_t)sinp | (uintptr_t)sb * es | (uintptr_t)sw * es) & (bytes - 1)) == 0; }
};

// the hidden states of the window [B, W, hidden] (element strides sb, sw) + q_proj.weight
struct KvpHidden {
    const void* p;
    int64_t sb, sw;
    const void* wq;
    int64_t hidden;
    // the two base pointers and the two strides of the hidden states
    bool aligned(size_t bytes, size_t es) const { return (((uintptr_t)p | (uintptr_t)wq | (uintptr_t)sb * es | (uintptr_t)sw * es) & (bytes - 1)) == 0; }
};

// One workspace layout = one sequence of take()s over the caller's buffer; every region starts on a multiple of 256 bytes.  A null
// base serves the size queries (the pointers are then null, bytes() is the same).  (topk_internal.h's TopkWsLayout stays word-based:
// it is __host__ __device__ and the cluster kernel derives addresses from it.)
struct KvpArena {
    char* base;
    size_t off = 0;
    explicit KvpArena(void* ws) : base(static_cast<char*>(ws)) {}
    template <class T> T* take(size_t count) {
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += kvp_align_up(count * sizeof(T), 256);
        return p;
    }
    size_t bytes() const { return off; }
};

// raise a kernel's dynamic LDS limit to `bytes` (above the 64 KiB a launch gets by default): KVP_OK, or KVP_EHIP with the message set
template <class Kernel> int kvp_raise_dynamic_lds(const char* who, Kernel* fn, size_t bytes) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess) return KVP_OK;
    kvp_set_error("%s: cannot raise the dynamic LDS limit to %zu bytes", who, bytes);
    return KVP_EHIP;
}

// ---- launchers shared between files ------------------------------------------------------------------------------------------
// rownorm.hip: out[b,h,s] = scale * ||x[b,h,s,:]||.  hist1 (may be null): also accumulate the select's first histogram; *hist1_done says
// whether the kernel that ran could.  _read_once: x is not read again soon (streaming loads).  rowsumsq2: sum_d k^2 and sum_d v^2 in one launch.
int kvp_rownorm_launch(KvpRows x, int dtype, int64_t B, int64_t H, int64_t S, int64_t D, float scale, float* out, hipStream_t stream,
                       uint32_t* hist1, bool* hist1_done);
int kvp_rownorm_launch_read_once(KvpRows x, int dtype, int64_t B, int64_t H, int64_t S, int64_t D, float scale, float* out, hipStream_t stream);
int kvp_rowsumsq2_launch(KvpRows k, KvpRows v, int dtype, int64_t B, int64_t H, int64_t S, int64_t D, float* out_k, float* out_v,
                         hipStream_t stream);
// gather.hip: K, V [B,H,S,D] -> contiguous K', V' [B,H,n,D] at idx [B,H,n] (the body of kvp_gather_kv)
int kvp_gather_launch(KvpRows k, KvpRows v, int dtype, int64_t B, int64_t H, int64_t S, int64_t D, const int32_t* idx, int64_t n, void* k_out,
                      void* v_out, hipStream_t stream);
// qproj.hip: RoPE'd window queries [B,Hq,W,D] from the hidden states and q_proj's weight
bool kvp_qproj_rope_eligible(int dtype, int64_t W, int64_t D, const KvpHidden& x, const KvpRope& r);
int kvp_qproj_rope_launch(const KvpHidden& x, const KvpRope& r, int dtype, int64_t B, int64_t Hq, void* out, hipStream_t stream);
