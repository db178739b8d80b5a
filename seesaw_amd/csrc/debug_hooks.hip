// Lab-bench entry points (include/seesaw_hip_debug.h): compiled into libseesaw_hip_debug.so only.
#ifndef SSW_DEBUG_HOOKS
#error "debug_hooks.hip belongs to the lab build (-DSSW_DEBUG_HOOKS)"
#endif
#include <algorithm>

#include "fb_handle.h"
#include "index_handle.h"

// ---------------------------------------------------------------------------------------
// A/B harness (tools/perf_gemm.py): time one variant on seeded operands and compare its
// output with variant 0 in the same process.
// ---------------------------------------------------------------------------------------
namespace {
__global__ void k_debug_fill(__bf16 *x, int64_t n, uint32_t seed, float scale) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        uint32_t h = (uint32_t)i * 2654435761u + seed;
        h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
        x[i] = (__bf16)(((int)(h & 0xffff) - 32768) * (scale / 32768.f));
    }
}
__global__ void k_debug_fill_f32(float *x, int64_t n, uint32_t seed, float scale) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        uint32_t h = (uint32_t)i * 2654435761u + seed;
        h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
        x[i] = ((int)(h & 0xffff) - 32768) * (scale / 32768.f);
    }
}
template <typename T>
__global__ void k_debug_maxdiff(const T *a, const T *b, int64_t n, float *out) {
    float m = 0.f;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float d = fabsf((float)a[i] - (float)b[i]);
        m = fmaxf(m, d == d ? d : 3.0e38f);
    }
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(reinterpret_cast<int *>(out), __float_as_int(m));
}
}  // namespace

extern "C" ssw_status ssw_tune_gemm(int32_t variant) {
    if (variant != 0 && variant != 2 && variant != 7 && variant != 9 && variant != 14 && variant != 15 && variant != 16 && variant != 17 &&
        !(variant >= 20 && variant <= 23)) {
        ssw::set_error("ssw_tune_gemm: variant %d unknown (0, 2, 7)", variant);
        return SSW_ERR_INVALID;
    }
    ssw::tune_gemm(variant);
    return SSW_OK;
}

// diagnostics of the persistent kernel (gemm_pw4.hip): mode 1 accumulates cycle stamps, read back here as
// out4 = {cycles in the mid-step wait + barrier, cycles in K-steps, K-steps, waves}; modes 2-4 are ablations
extern "C" ssw_status ssw_debug_gemm_pw4_mode(int32_t mode, uint64_t *out6_or_null) {
    ssw::gemm_pw4_set_mode(mode);
    if (out6_or_null) return ssw::gemm_pw4_read_diag(reinterpret_cast<unsigned long long *>(out6_or_null), true);
    return SSW_OK;
}

extern "C" ssw_status ssw_debug_gemm_pw4_wg(uint64_t *out4096) {
    return ssw::gemm_pw4_read_wg(reinterpret_cast<unsigned long long *>(out4096));
}

extern "C" ssw_status ssw_debug_gemm(int32_t M, int32_t N, int32_t K, int32_t epi, int32_t variant, int32_t iters,
                                     float *out_ms, float *out_maxdiff) {
    using namespace ssw;
    if (M <= 0 || iters <= 0 || epi < 0 || epi > 7) {
        set_error("ssw_debug_gemm: bad arguments");
        return SSW_ERR_INVALID;
    }
    if (epi >= 4) {  // the LayerNorm-folded consumers (4, 5) and the row producers (6, 7): timing only, filled operands
        __bf16 *A = nullptr, *W = nullptr, *xc = nullptr;
        float *bias = nullptr, *c1 = nullptr, *st_in = nullptr, *st_out = nullptr;
        void *res = nullptr, *C = nullptr;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        const int np_in = K / 128;
        auto cleanup = [&]() {
            for (void *p : {(void *)A, (void *)W, (void *)xc, (void *)bias, (void *)c1, (void *)st_in, (void *)st_out, res, C}) (void)hipFree(p);
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
        };
        bool ok = hipMalloc(&A, (size_t)M * K * 2) == hipSuccess && hipMalloc(&W, (size_t)N * K * 2) == hipSuccess &&
                  hipMalloc(&xc, (size_t)M * N * 2) == hipSuccess && hipMalloc(&bias, (size_t)N * 4) == hipSuccess &&
                  hipMalloc(&c1, (size_t)N * 4) == hipSuccess && hipMalloc(&st_in, (size_t)M * np_in * 8) == hipSuccess &&
                  hipMalloc(&st_out, (size_t)M * (N / 128 + 1) * 8) == hipSuccess && hipMalloc(&res, (size_t)M * N * 4) == hipSuccess &&
                  hipMalloc(&C, (size_t)M * N * 4) == hipSuccess && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess;
        if (!ok) {
            cleanup();
            set_error("ssw_debug_gemm: allocation failed");
            return SSW_ERR_HIP;
        }
        hipLaunchKernelGGL(k_debug_fill, dim3(2048), dim3(256), 0, 0, A, (int64_t)M * K, 0x1234u, 1.0f);
        hipLaunchKernelGGL(k_debug_fill, dim3(2048), dim3(256), 0, 0, W, (int64_t)N * K, 0x9876u, 0.05f);
        hipLaunchKernelGGL(k_debug_fill_f32, dim3(64), dim3(256), 0, 0, bias, (int64_t)N, 0x4242u, 0.5f);
        hipLaunchKernelGGL(k_debug_fill_f32, dim3(64), dim3(256), 0, 0, c1, (int64_t)N, 0x4243u, 0.5f);
        hipLaunchKernelGGL(k_debug_fill_f32, dim3(2048), dim3(256), 0, 0, (float *)res, (int64_t)M * N, 0x7777u, 1.0f);
        (void)hipMemsetAsync(st_in, 0, (size_t)M * np_in * 8, 0);  // mean 0, variance 0: rstd = 1 / sqrt(eps)
        GemmLn ln;
        ln.stats_in = st_in; ln.np_in = np_in; ln.inv_dim = 1.f / K; ln.eps = 1.f; ln.c1 = c1;
        ln.xcopy = xc; ln.stats_out = st_out;
        const int keep = gemm_variant();
        tune_gemm(variant);
        int rc = launch_gemm_bf16_ln(epi, 0, A, W, bias, (const float *)res, C, M, N, K, ln);
        (void)hipEventRecord(e0, 0);
        for (int i = 0; i < iters && rc == SSW_OK; ++i) rc = launch_gemm_bf16_ln(epi, 0, A, W, bias, (const float *)res, C, M, N, K, ln);
        (void)hipEventRecord(e1, 0);
        tune_gemm(keep);
        float ms = 0.f;
        if (rc == SSW_OK && (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess)) rc = SSW_ERR_HIP;
        cleanup();
        if (out_ms) *out_ms = ms / iters;
        if (out_maxdiff) *out_maxdiff = 0.f;
        return (ssw_status)rc;
    }
    const bool out_bf16 = (epi == 1 || epi == 2);
    const size_t out_bytes = (size_t)M * N * (out_bf16 ? 2 : 4);
    __bf16 *A = nullptr, *W = nullptr;
    float *bias = nullptr, *res = nullptr, *diff = nullptr;
    void *c_ref = nullptr, *c_var = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = SSW_OK;
    auto cleanup = [&]() {
        for (void *p : {(void *)A, (void *)W, (void *)bias, (void *)res, (void *)diff, c_ref, c_var}) (void)hipFree(p);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    };
#define SSW_DBG_TRY(expr)                                                      \
    if (hipError_t _e = (expr); _e != hipSuccess) {                            \
        set_error("%s failed: %s", #expr, hipGetErrorString(_e));              \
        cleanup();                                                             \
        return SSW_ERR_HIP;                                                    \
    }
    SSW_DBG_TRY(hipMalloc(&A, (size_t)M * K * 2));
    SSW_DBG_TRY(hipMalloc(&W, (size_t)N * K * 2));
    SSW_DBG_TRY(hipMalloc(&bias, (size_t)N * 4));
    SSW_DBG_TRY(hipMalloc(&res, (size_t)M * N * 4));
    SSW_DBG_TRY(hipMalloc(&diff, 4));
    SSW_DBG_TRY(hipMalloc(&c_ref, out_bytes));
    SSW_DBG_TRY(hipMalloc(&c_var, out_bytes));
    hipLaunchKernelGGL(k_debug_fill, dim3(2048), dim3(256), 0, 0, A, (int64_t)M * K, 0x1234u, 1.0f);
    hipLaunchKernelGGL(k_debug_fill, dim3(2048), dim3(256), 0, 0, W, (int64_t)N * K, 0x9876u, 0.05f);
    hipLaunchKernelGGL(k_debug_fill_f32, dim3(64), dim3(256), 0, 0, bias, (int64_t)N, 0x4242u, 0.5f);
    hipLaunchKernelGGL(k_debug_fill_f32, dim3(2048), dim3(256), 0, 0, res, (int64_t)M * N, 0x7777u, 1.0f);
    SSW_DBG_TRY(hipMemsetAsync(diff, 0, 4, 0));
    SSW_DBG_TRY(hipEventCreate(&e0));
    SSW_DBG_TRY(hipEventCreate(&e1));
    const int keep = gemm_variant();
    tune_gemm(0);
    rc = launch_gemm_bf16_nt(epi, 0, A, W, bias, res, c_ref, M, N, K);
    tune_gemm(variant);
    if (rc == SSW_OK) rc = launch_gemm_bf16_nt(epi, 0, A, W, bias, res, c_var, M, N, K);  // warm-up + checked run
    if (rc == SSW_OK) {
        if (out_bf16)
            hipLaunchKernelGGL(k_debug_maxdiff<__bf16>, dim3(1024), dim3(256), 0, 0, (const __bf16 *)c_ref,
                               (const __bf16 *)c_var, (int64_t)M * N, diff);
        else
            hipLaunchKernelGGL(k_debug_maxdiff<float>, dim3(1024), dim3(256), 0, 0, (const float *)c_ref,
                               (const float *)c_var, (int64_t)M * N, diff);
        (void)hipEventRecord(e0, 0);
        for (int i = 0; i < iters && rc == SSW_OK; ++i) rc = launch_gemm_bf16_nt(epi, 0, A, W, bias, res, c_var, M, N, K);
        (void)hipEventRecord(e1, 0);
    }
    tune_gemm(keep);
    if (rc != SSW_OK) {
        cleanup();
        return rc;
    }
    SSW_DBG_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    SSW_DBG_TRY(hipEventElapsedTime(&ms, e0, e1));
    if (out_ms) *out_ms = ms / iters;
    if (out_maxdiff) SSW_DBG_TRY(hipMemcpy(out_maxdiff, diff, 4, hipMemcpyDeviceToHost));
#undef SSW_DBG_TRY
    cleanup();
    return SSW_OK;
}


// ---------------------------------------------------------------------------------------
// one product / one fused launch on the caller's operands (tests/test_gemm_gpu.py)
// ---------------------------------------------------------------------------------------
namespace {
struct DevBufs {
    std::vector<void *> ptrs;
    ~DevBufs() {
        for (void *p : ptrs) (void)hipFree(p);
    }
    ssw_status up(const void *host, size_t bytes, void **dev, bool copy = true) {
        *dev = nullptr;
        SSW_HIP_TRY(hipMalloc(dev, bytes ? bytes : 16));
        ptrs.push_back(*dev);
        if (host && copy) SSW_HIP_TRY(hipMemcpy(*dev, host, bytes, hipMemcpyHostToDevice));
        else SSW_HIP_TRY(hipMemset(*dev, 0xFF, bytes));  // NaN patterns: an element the kernel skips shows
        return SSW_OK;
    }
};
}  // namespace

extern "C" ssw_status ssw_debug_gemm_run(int32_t epi, int32_t variant, int32_t M, int32_t N, int32_t K, const uint16_t *A_bf16,
                                         const uint16_t *W_bf16, const float *bias_or_c2, const float *residual_or_null,
                                         uint16_t *xcopy_inout_or_null, const float *stats_in_or_null, int32_t np_in,
                                         const float *c1_or_null, float inv_dim, float eps, void *C_out_or_null,
                                         float *stats_out_or_null) {
    using namespace ssw;
    SSW_REQUIRE(epi >= 0 && epi <= 10 && M > 0 && N > 0 && K > 0 && A_bf16 && W_bf16, "ssw_debug_gemm_run: bad arguments");
    if (epi == 9 || epi == 10) {
        // 9: the producer epilogue behind a split-K product (launch_gemm_splitk_stats: the text tower's fc2), `variant` = splits;
        // 10: the producer epilogue with the residual rows at a stride (GemmLn::res_ld: the pooled last layer's out-projection),
        //     `variant` = S: residual_or_null holds M * S rows of N, row m S is added to row m of the product
        SSW_REQUIRE(bias_or_c2 && residual_or_null && xcopy_inout_or_null && C_out_or_null && stats_out_or_null && variant >= 1,
                    "ssw_debug_gemm_run: the producer forms need bias, residual, the copy, the output, the statistics and splits / S >= 1");
        DevBufs d9;
        void *A9, *W9, *b9, *r9, *x9, *C9, *s9, *P9 = nullptr;
        const int64_t res_rows = epi == 10 ? (int64_t)M * variant : M;
        SSW_TRY(d9.up(A_bf16, (size_t)M * K * 2, &A9));
        SSW_TRY(d9.up(W_bf16, (size_t)N * K * 2, &W9));
        SSW_TRY(d9.up(bias_or_c2, (size_t)N * 4, &b9));
        SSW_TRY(d9.up(residual_or_null, (size_t)res_rows * N * 4, &r9));
        SSW_TRY(d9.up(nullptr, (size_t)M * N * 2, &x9));
        SSW_TRY(d9.up(nullptr, (size_t)M * N * 4, &C9));
        SSW_TRY(d9.up(nullptr, (size_t)M * (N / 128) * 2 * 4, &s9));
        GemmLn ln;
        ln.xcopy = (__bf16 *)x9;
        ln.stats_out = (float *)s9;
        if (epi == 9) {
            SSW_TRY(d9.up(nullptr, (size_t)variant * M * N * 4, &P9));
            SSW_TRY(launch_gemm_splitk_stats(0, A9, W9, (const float *)b9, (const float *)r9, (float *)C9, (float *)P9, M, N, K, variant, ln));
        } else {
            ln.res_ld = (int64_t)variant * N;
            SSW_TRY(launch_gemm_bf16_ln(6, 0, A9, W9, (const float *)b9, (const float *)r9, C9, M, N, K, ln));
        }
        SSW_HIP_TRY(hipDeviceSynchronize());
        SSW_HIP_TRY(hipMemcpy(C_out_or_null, C9, (size_t)M * N * 4, hipMemcpyDeviceToHost));
        SSW_HIP_TRY(hipMemcpy(xcopy_inout_or_null, x9, (size_t)M * N * 2, hipMemcpyDeviceToHost));
        SSW_HIP_TRY(hipMemcpy(stats_out_or_null, s9, (size_t)M * (N / 128) * 2 * 4, hipMemcpyDeviceToHost));
        return SSW_OK;
    }
    if (epi == 8) {  // the split-K product of few-tile shapes (launch_gemm_splitk_f32): `variant` = number of splits
        SSW_REQUIRE(bias_or_c2 && C_out_or_null && variant >= 1, "ssw_debug_gemm_run: split-K needs bias, an output and the split count");
        DevBufs d8;
        void *A8, *W8, *b8, *r8 = nullptr, *C8, *P8;
        SSW_TRY(d8.up(A_bf16, (size_t)M * K * 2, &A8));
        SSW_TRY(d8.up(W_bf16, (size_t)N * K * 2, &W8));
        SSW_TRY(d8.up(bias_or_c2, (size_t)N * 4, &b8));
        if (residual_or_null) SSW_TRY(d8.up(residual_or_null, (size_t)M * N * 4, &r8));
        SSW_TRY(d8.up(nullptr, (size_t)M * N * 4, &C8));
        SSW_TRY(d8.up(nullptr, (size_t)variant * M * N * 4, &P8));
        SSW_TRY(launch_gemm_splitk_f32(0, A8, W8, (const float *)b8, (const float *)r8, (float *)C8, (float *)P8, M, N, K, variant));
        SSW_HIP_TRY(hipDeviceSynchronize());
        SSW_HIP_TRY(hipMemcpy(C_out_or_null, C8, (size_t)M * N * 4, hipMemcpyDeviceToHost));
        return SSW_OK;
    }
    const bool c_bf16 = epi == 1 || epi == 2 || epi == 4 || epi == 5, c_f32 = epi == 0 || epi == 3 || epi == 6;
    const size_t mn = (size_t)M * N;
    const int n_tiles = N / 128;
    DevBufs d;
    void *A, *W, *bias = nullptr, *res = nullptr, *xc = nullptr, *sin = nullptr, *c1 = nullptr, *C = nullptr, *sout = nullptr;
    SSW_TRY(d.up(A_bf16, (size_t)M * K * 2, &A));
    SSW_TRY(d.up(W_bf16, (size_t)N * K * 2, &W));
    if (bias_or_c2) SSW_TRY(d.up(bias_or_c2, (size_t)N * 4, &bias));
    if (residual_or_null) SSW_TRY(d.up(residual_or_null, mn * 4, &res));
    if (xcopy_inout_or_null) SSW_TRY(d.up(xcopy_inout_or_null, mn * 2, &xc, epi == 7));
    if (stats_in_or_null) SSW_TRY(d.up(stats_in_or_null, (size_t)M * np_in * 2 * 4, &sin));
    if (c1_or_null) SSW_TRY(d.up(c1_or_null, (size_t)N * 4, &c1));
    if (c_bf16 || c_f32) SSW_TRY(d.up(nullptr, mn * (c_bf16 ? 2 : 4), &C));
    if (epi >= 6) SSW_TRY(d.up(nullptr, (size_t)M * n_tiles * 2 * 4, &sout));
    const int keep = gemm_variant();
    if (variant >= 0) tune_gemm(variant);
    ssw_status rc;
    if (epi <= 3) {
        rc = launch_gemm_bf16_nt(epi, 0, A, W, (const float *)bias, (const float *)res, C, M, N, K);
    } else {
        GemmLn ln;
        ln.stats_in = (const float *)sin;
        ln.np_in = np_in;
        ln.inv_dim = inv_dim;
        ln.eps = eps;
        ln.c1 = (const float *)c1;
        ln.xcopy = (__bf16 *)xc;
        ln.stats_out = (float *)sout;
        rc = launch_gemm_bf16_ln(epi, 0, A, W, (const float *)bias, (const float *)res, C, M, N, K, ln);
    }
    tune_gemm(keep);
    if (rc != SSW_OK) return rc;
    SSW_HIP_TRY(hipDeviceSynchronize());
    if (C && C_out_or_null) SSW_HIP_TRY(hipMemcpy(C_out_or_null, C, mn * (c_bf16 ? 2 : 4), hipMemcpyDeviceToHost));
    if (xc && epi >= 6) SSW_HIP_TRY(hipMemcpy(xcopy_inout_or_null, xc, mn * 2, hipMemcpyDeviceToHost));
    if (sout && stats_out_or_null) SSW_HIP_TRY(hipMemcpy(stats_out_or_null, sout, (size_t)M * n_tiles * 2 * 4, hipMemcpyDeviceToHost));
    return SSW_OK;
}

extern "C" ssw_status ssw_debug_attn_out_run(int32_t B, int32_t S, const uint16_t *qkv_bf16, const uint16_t *Wo_bf16,
                                             const float *bo, uint16_t *xcopy_inout, const float *res_in_or_null,
                                             float *res_out_or_null, float *stats_out, float scale) {
    using namespace ssw;
    SSW_REQUIRE(B > 0 && qkv_bf16 && Wo_bf16 && bo && xcopy_inout && stats_out, "ssw_debug_attn_out_run: NULL argument");
    SSW_REQUIRE((res_in_or_null == nullptr) == (res_out_or_null == nullptr), "f32 stream: both residual pointers");
    const int D = 768, H = 12;
    const size_t rows = (size_t)B * S;
    DevBufs d;
    void *qkv, *wo, *wo_pk, *b, *xc, *rin = nullptr, *rout = nullptr, *st;
    SSW_TRY(d.up(qkv_bf16, rows * 3 * D * 2, &qkv));
    SSW_TRY(d.up(Wo_bf16, (size_t)D * D * 2, &wo));
    SSW_TRY(d.up(nullptr, (size_t)D * D * 2, &wo_pk));
    SSW_TRY(d.up(bo, (size_t)D * 4, &b));
    SSW_TRY(d.up(xcopy_inout, rows * D * 2, &xc, res_in_or_null == nullptr));
    if (res_in_or_null) {
        SSW_TRY(d.up(res_in_or_null, rows * D * 4, &rin));
        SSW_TRY(d.up(nullptr, rows * D * 4, &rout));
    }
    SSW_TRY(d.up(nullptr, rows * 4 * 4, &st));
    SSW_TRY(pack_attn_outproj_weight(0, wo, wo_pk));
    SSW_TRY(launch_attn_outproj(0, qkv, wo_pk, (const float *)b, xc, (const float *)rin, (float *)rout, (float *)st, B, S, D, H, scale));
    SSW_HIP_TRY(hipDeviceSynchronize());
    SSW_HIP_TRY(hipMemcpy(xcopy_inout, xc, rows * D * 2, hipMemcpyDeviceToHost));
    if (rout) SSW_HIP_TRY(hipMemcpy(res_out_or_null, rout, rows * D * 4, hipMemcpyDeviceToHost));
    SSW_HIP_TRY(hipMemcpy(stats_out, st, rows * 4 * 4, hipMemcpyDeviceToHost));
    return SSW_OK;
}

extern "C" ssw_status ssw_debug_attn_out_stamps(uint64_t *out, int32_t n_words) {
    SSW_REQUIRE(out && n_words > 0 && n_words <= 32 * 1024, "ssw_debug_attn_out_stamps: bad arguments");
    return ssw::read_ao_stamps(out, n_words);
}

// ---------------------------------------------------------------------------------------
// The index's certified pre-scan, step by step (csrc/index_prune.hip; the handle: index_handle.h).
// ---------------------------------------------------------------------------------------
using namespace ssw;

static ssw_status require_shadow(ssw_index *idx, const char *who, ShadowKind kind = SHADOW_Q8) {
    bool ready = false;
    SSW_TRY(ensure_shadow(idx, kind, &ready));
    if (!ready) {
        set_error("%s: the shadow was refused for memory", who);
        return SSW_ERR_NOMEM;
    }
    return SSW_OK;
}

static bool shadow_current(const ssw_index *idx, ShadowKind kind) {
    return idx->prune.sh[kind].codes && !idx->prune.sh[kind].stale;
}

// what the threshold selection leaves behind, written by hand: k keys (only the k-th is read) and [count, overflow]
static ssw_status stand_in_threshold(ssw_index *idx, float threshold, int32_t k, int32_t sel_count, int32_t sel_overflow) {
    std::vector<uint64_t> keys((size_t)k, (uint64_t)f32_to_ord(threshold) << 32);
    const int32_t count[2] = {sel_count, sel_overflow};
    SSW_HIP_TRY(hipMemcpyAsync(idx->ws.out_keys, keys.data(), keys.size() * sizeof(uint64_t), hipMemcpyHostToDevice,
                               idx->stream));
    SSW_HIP_TRY(hipMemcpyAsync(idx->ws.out_count, count, sizeof(count), hipMemcpyHostToDevice, idx->stream));
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));  // keys and count are pageable host memory
    return SSW_OK;
}

extern "C" {

// ---- the pre-scan's intermediate state (tests/test_prune_certificate_gpu.py) ----------------------------------------
// Each hook drives the product's kernels through the steps scan_for_topk is made of, on the index's own buffers.
ssw_status ssw_debug_prune_shadow(ssw_index *idx, int64_t first_row, int64_t n_rows, int8_t *out_codes, float *out_scale,
                                  float *out_err) {
    SSW_REQUIRE(idx != nullptr, "idx is NULL");
    SSW_REQUIRE(first_row >= 0 && n_rows >= 0 && first_row + n_rows <= idx->n, "rows [%lld, +%lld) outside [0, %lld)",
                (long long)first_row, (long long)n_rows, (long long)idx->n);
    SSW_REQUIRE(prune_eligible(idx), "the index is not pruned (ssw_tune_prune, dim, borrowed or escaped rows)");
    DeviceGuard guard(idx->device);
    SSW_TRY(require_shadow(idx, "prune_shadow"));
    if (n_rows > 0 && out_codes)
        SSW_HIP_TRY(hipMemcpyAsync(out_codes, idx->prune.sh[SHADOW_Q8].codes + first_row * idx->dim, (size_t)n_rows * idx->dim,
                                   hipMemcpyDeviceToHost, idx->stream));
    if (n_rows > 0 && out_scale)
        SSW_HIP_TRY(hipMemcpyAsync(out_scale, idx->prune.sh[SHADOW_Q8].scale + first_row, (size_t)n_rows * sizeof(float),
                                   hipMemcpyDeviceToHost, idx->stream));
    if (n_rows > 0 && out_err)
        SSW_HIP_TRY(hipMemcpyAsync(out_err, idx->prune.sh[SHADOW_Q8].err + first_row, (size_t)n_rows * sizeof(float),
                                   hipMemcpyDeviceToHost, idx->stream));
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    return SSW_OK;
}

ssw_status ssw_debug_prune_bounds(ssw_index *idx, const float *q_host, float *out_lb, float *out_Q,
                                  int32_t *out_unbounded) {
    SSW_REQUIRE(idx != nullptr && q_host != nullptr && out_lb != nullptr && out_Q != nullptr && out_unbounded != nullptr,
                "NULL argument");
    SSW_TRY(check_query(idx, q_host));
    SSW_REQUIRE(prune_eligible(idx), "the index is not pruned (ssw_tune_prune, dim, borrowed or escaped rows)");
    DeviceGuard guard(idx->device);
    SSW_TRY(require_shadow(idx, "prune_bounds"));
    SSW_TRY(idx->q_stage.push(idx->q_dev, q_host, (size_t)idx->dim * sizeof(float), idx->stream));
    SSW_TRY(prune_bounds(idx, SHADOW_Q8, idx->q_dev, nullptr));  // as in scan_for_topk: every reader completes the buffer with the scan of q_last
    unsigned state[4] = {0u, 0u, 0u, 0u};
    SSW_HIP_TRY(hipMemcpyAsync(state, idx->prune.state, sizeof(state), hipMemcpyDeviceToHost, idx->stream));
    SSW_HIP_TRY(hipMemcpyAsync(out_lb, idx->scores, (size_t)idx->n * sizeof(float), hipMemcpyDeviceToHost, idx->stream));
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    memcpy(out_Q, &state[1], sizeof(float));
    *out_unbounded = (int32_t)state[2];
    return SSW_OK;
}

ssw_status ssw_debug_prune_survivors(ssw_index *idx, float threshold, int32_t k, int32_t sel_count, int32_t sel_overflow,
                                     int64_t cap, int32_t *out_published, int64_t *out_collected, int64_t *out_rows) {
    SSW_REQUIRE(idx != nullptr && out_published != nullptr && out_collected != nullptr, "NULL argument");
    SSW_REQUIRE(k >= 1 && k <= SSW_MAX_TOPK, "k=%d outside [1, %d]", k, SSW_MAX_TOPK);
    SSW_REQUIRE(cap >= 0 && cap <= SURV_CAP, "cap=%lld outside [0, %lld]", (long long)cap, (long long)SURV_CAP);
    SSW_REQUIRE(cap == 0 || out_rows != nullptr, "out_rows is NULL");
    SSW_REQUIRE(idx->scores_partial && shadow_current(idx, SHADOW_Q8), "no bounds in the buffer: ssw_debug_prune_bounds first");
    DeviceGuard guard(idx->device);
    SSW_TRY(ensure_ws(idx));
    SSW_HIP_TRY(hipMemsetAsync(idx->prune.state, 0, sizeof(unsigned), idx->stream));  // the counter k_q8_query resets
    SSW_TRY(stand_in_threshold(idx, threshold, k, sel_count, sel_overflow));
    int32_t m = -1;
    SSW_TRY(prune_survivors(idx, SHADOW_Q8, k, cap, nullptr, &m));
    unsigned collected = 0u;
    SSW_HIP_TRY(hipMemcpyAsync(&collected, idx->prune.state, sizeof(unsigned), hipMemcpyDeviceToHost, idx->stream));
    if (m > 0)
        SSW_HIP_TRY(hipMemcpyAsync(out_rows, idx->prune.surv_rows, (size_t)m * sizeof(int64_t), hipMemcpyDeviceToHost,
                                   idx->stream));
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    *out_published = m;
    *out_collected = (int64_t)collected;
    return SSW_OK;
}

ssw_status ssw_debug_prune_scan_mq_shape(ssw_index *idx, int32_t *out_blocks, int32_t *out_tiles) {
    SSW_REQUIRE(idx != nullptr && out_blocks != nullptr && out_tiles != nullptr, "NULL argument");
    SSW_REQUIRE(q8_dim_supported(idx->dim), "dim=%d has no shadow scan", idx->dim);
    int blocks = 0, tiles = 0;
    scan_shape(SCAN_Q8_MQ, idx->dim, idx->device, idx->n, &blocks, &tiles);
    *out_blocks = blocks;
    *out_tiles = tiles;
    return SSW_OK;
}

static ssw_status require_shadow6(ssw_index *idx, const char *who);

// the chunk's buffers for nq queries staged from the host, for the hooks below; six: on the 6-bit shadow
static ssw_status debug_chunk_ready(ssw_index *idx, int32_t nq, bool six = false) {
    if (six) {
        SSW_TRY(require_shadow6(idx, "prune6_bounds_mq"));
    } else {
        SSW_REQUIRE(prune_batch_eligible(idx), "the index is not pruned (ssw_tune_prune, dim, borrowed or escaped rows)");
        SSW_TRY(require_shadow(idx, "prune_bounds_mq"));
    }
    idx->prune_batch.kind = six ? SHADOW_Q6 : SHADOW_Q8;  // what prune_batch_shadow would have left
    SSW_TRY(ensure_ws(idx));
    int w = 0;
    SSW_TRY(batch_buffers(idx, nq, true, &w));
    if (w == nq && idx->batch.qb_dev) SSW_TRY(ensure_prune_batch(idx, nq, &w));
    if (w != nq || !idx->batch.qb_dev) {
        set_error("prune_bounds_mq: no memory for a chunk of %d queries", nq);
        return SSW_ERR_NOMEM;
    }
    return SSW_OK;
}

ssw_status ssw_debug_prune_bounds_mq(ssw_index *idx, const float *q_host, int32_t nq, int32_t *out_I_hi, int32_t *out_I_lo,
                                     float *out_lb, float *out_Qe, int8_t *out_codes) {
    SSW_REQUIRE(idx != nullptr && q_host != nullptr, "NULL argument");
    SSW_REQUIRE(nq >= 1 && nq <= Q8_MQ_WIDTH, "nq=%d outside [1, %d]", nq, Q8_MQ_WIDTH);
    DeviceGuard guard(idx->device);
    SSW_TRY(debug_chunk_ready(idx, nq));
    PruneBatchState &pb = idx->prune_batch;
    const size_t dim = (size_t)idx->dim, cells = (size_t)nq * idx->n;
    int32_t *dbg = nullptr;
    if (out_I_hi || out_I_lo) SSW_HIP_TRY(hipMalloc((void **)&dbg, 2 * cells * sizeof(int32_t)));
    std::vector<unsigned> mq((size_t)Q8_MQ_WIDTH * Q8_MQ_WORDS);
    std::vector<int8_t> planes(q8_mq_plane_bytes(idx->dim));
    auto run = [&]() -> ssw_status {
        SSW_TRY(idx->batch.qb_stage.push(idx->batch.qb_dev, q_host, (size_t)nq * dim * sizeof(float), idx->stream));
        SSW_TRY(prune_bounds_mq(idx, nq, dbg, dbg ? dbg + cells : nullptr));
        if (out_I_hi) SSW_HIP_TRY(hipMemcpyAsync(out_I_hi, dbg, cells * sizeof(int32_t), hipMemcpyDeviceToHost, idx->stream));
        if (out_I_lo)
            SSW_HIP_TRY(hipMemcpyAsync(out_I_lo, dbg + cells, cells * sizeof(int32_t), hipMemcpyDeviceToHost, idx->stream));
        if (out_lb)
            for (int j = 0; j < nq; ++j)
                SSW_HIP_TRY(hipMemcpyAsync(out_lb + (size_t)j * idx->n, chunk_slab(idx, nq, j), (size_t)idx->n * sizeof(float),
                                           hipMemcpyDeviceToHost, idx->stream));
        SSW_HIP_TRY(hipMemcpyAsync(mq.data(), pb.mq, mq.size() * sizeof(unsigned), hipMemcpyDeviceToHost, idx->stream));
        SSW_HIP_TRY(hipMemcpyAsync(planes.data(), pb.planes, planes.size(), hipMemcpyDeviceToHost, idx->stream));
        SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
        return SSW_OK;
    };
    const ssw_status st = run();
    if (st != SSW_OK) (void)hipStreamSynchronize(idx->stream);
    (void)hipFree(dbg);
    SSW_TRY(st);
    for (int j = 0; j < nq; ++j) {
        const unsigned *w = mq.data() + (size_t)j * Q8_MQ_WORDS;
        if (out_Qe) {
            memcpy(out_Qe + 4 * j, &w[1], 4);      // Q
            memcpy(out_Qe + 4 * j + 1, &w[3], 4);  // e
            memcpy(out_Qe + 4 * j + 2, &w[4], 4);  // t2
            out_Qe[4 * j + 3] = (float)w[2];       // 1 = the query cannot be bounded
        }
        if (out_codes)  // the planes' fragment order (prune.hip) back to natural element order
            for (int pl = 0; pl < 2; ++pl)
                for (size_t i = 0; i < dim; ++i)
                    out_codes[((size_t)j * 2 + pl) * dim + i] =
                        planes[(((i >> 6) * 2 + pl) * 64 + ((i & 63) >> 4) * 16 + j) * 16 + (i & 15)];
    }
    return SSW_OK;
}

ssw_status ssw_debug_prune_survivors_mq(ssw_index *idx, int32_t nq, int32_t slot, float threshold, int32_t k,
                                        int32_t sel_count, int32_t sel_overflow, int64_t cap, int32_t *out_published,
                                        int64_t *out_collected, int64_t *out_rows) {
    SSW_REQUIRE(idx != nullptr && out_published != nullptr && out_collected != nullptr, "NULL argument");
    SSW_REQUIRE(nq >= 1 && nq <= Q8_MQ_WIDTH && slot >= 0 && slot < nq, "slot=%d outside the chunk of %d", slot, nq);
    SSW_REQUIRE(k >= 1 && k <= SSW_MAX_TOPK, "k=%d outside [1, %d]", k, SSW_MAX_TOPK);
    SSW_REQUIRE(cap >= 0 && cap <= SURV_CAP, "cap=%lld outside [0, %lld]", (long long)cap, (long long)SURV_CAP);
    SSW_REQUIRE(cap == 0 || out_rows != nullptr, "out_rows is NULL");
    PruneBatchState &pb = idx->prune_batch;
    SSW_REQUIRE(idx->scores_partial && pb.kind == SHADOW_Q8 && shadow_current(idx, SHADOW_Q8) && pb.slots >= nq &&
                    idx->batch.side_slabs >= nq - 1,
                "no bounds of such a chunk in the buffers: ssw_debug_prune_bounds_mq first");
    DeviceGuard guard(idx->device);
    SSW_TRY(ensure_ws(idx));
    unsigned *st = pb.mq + slot * Q8_MQ_WORDS;
    SSW_HIP_TRY(hipMemsetAsync(st, 0, sizeof(unsigned), idx->stream));      // the counter and the "selection failed"
    SSW_HIP_TRY(hipMemsetAsync(st + 5, 0, sizeof(unsigned), idx->stream));  // word k_q8_query_mq resets
    SSW_TRY(stand_in_threshold(idx, threshold, k, sel_count, sel_overflow));
    SSW_TRY(prune_survivors_slot(idx, nq, slot, k, cap));
    int32_t m[Q8_MQ_WIDTH];
    SSW_TRY(prune_publish_mq(idx, nq, cap, nullptr, m));
    unsigned collected = 0u;
    SSW_HIP_TRY(hipMemcpyAsync(&collected, st, sizeof(unsigned), hipMemcpyDeviceToHost, idx->stream));
    if (m[slot] > 0)
        SSW_HIP_TRY(hipMemcpyAsync(out_rows, pb.surv_rows + (int64_t)slot * SURV_CAP, (size_t)m[slot] * sizeof(int64_t),
                                   hipMemcpyDeviceToHost, idx->stream));
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    *out_published = m[slot];
    *out_collected = (int64_t)collected;
    return SSW_OK;
}

// ---- the device-sized rescoring alone (rescore_dev.hip; tests/test_rescore_dev_gpu.py) --------------------------------
__global__ void k_fill_u32(unsigned *__restrict__ p, int64_t n, unsigned v) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = v;
}

ssw_status ssw_debug_rescore_survivors(ssw_index *idx, const float *q_host, int32_t nq, const int64_t *rows_host,
                                       const int64_t *counts, const int32_t *fail_bits, float *out_slabs_host,
                                       int32_t *out_waves) {
    SSW_REQUIRE(idx && q_host && counts && fail_bits && out_slabs_host && out_waves, "NULL argument");
    SSW_REQUIRE(nq >= 1 && nq <= Q8_MQ_WIDTH, "nq=%d outside [1, %d]", nq, Q8_MQ_WIDTH);
    SSW_REQUIRE(q6_dim_supported(idx->dim) && idx->n >= 1, "dim=%d or n=%lld has no pruned chunk", idx->dim, (long long)idx->n);
    const int64_t cap = batch_dev_surv_cap();
    int64_t listed = 0;
    for (int j = 0; j < nq; ++j) {
        SSW_REQUIRE(counts[j] >= 0 && counts[j] <= 0x7fffffff, "counts[%d]=%lld", j, (long long)counts[j]);
        listed += std::min(counts[j], cap);
    }
    SSW_REQUIRE(listed == 0 || rows_host != nullptr, "rows_host is NULL");
    for (int64_t i = 0; i < listed; ++i)
        SSW_REQUIRE(rows_host[i] >= 0 && rows_host[i] < idx->n, "rows_host[%lld]=%lld outside [0, %lld)", (long long)i,
                    (long long)rows_host[i], (long long)idx->n);
    DeviceGuard guard(idx->device);
    int w = 0;
    SSW_TRY(batch_buffers(idx, nq, true, &w));
    if (w == nq && idx->batch.qb_dev) SSW_TRY(ensure_prune_batch(idx, nq, &w));
    if (w != nq || !idx->batch.qb_dev) {
        set_error("rescore_survivors: no memory for a chunk of %d queries", nq);
        return SSW_ERR_NOMEM;
    }
    PruneBatchState &pb = idx->prune_batch;
    pb.dev_w = 0;
    std::vector<unsigned> mq((size_t)Q8_MQ_WIDTH * Q8_MQ_WORDS, 0u);
    const size_t dim = (size_t)idx->dim;
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));  // the copies below read pageable host memory
    const int64_t *list = rows_host;
    for (int j = 0; j < nq; ++j) {
        unsigned *st = mq.data() + (size_t)j * Q8_MQ_WORDS;
        st[0] = (unsigned)counts[j];
        st[5] = (unsigned)(fail_bits[j] & 1);
        st[2] = (unsigned)((fail_bits[j] >> 1) & 1);
        const int64_t m = std::min(counts[j], cap);
        if (m > 0)
            SSW_HIP_TRY(hipMemcpyAsync(pb.surv_rows + (int64_t)j * SURV_CAP, list, (size_t)m * sizeof(int64_t),
                                       hipMemcpyHostToDevice, idx->stream));
        list += m;
        hipLaunchKernelGGL(k_fill_u32, dim3(256), dim3(256), 0, idx->stream,
                           reinterpret_cast<unsigned *>(chunk_slab(idx, nq, j)), idx->n, 0x7FC0BEEFu);
        SSW_HIP_TRY(hipGetLastError());
    }
    SSW_HIP_TRY(hipMemcpyAsync(pb.mq, mq.data(), mq.size() * sizeof(unsigned), hipMemcpyHostToDevice, idx->stream));
    SSW_HIP_TRY(hipMemcpyAsync(idx->batch.qb_dev, q_host, (size_t)nq * dim * sizeof(float), hipMemcpyHostToDevice, idx->stream));
    SSW_TRY(rescore_survivors_chunk(idx, nq, cap));
    for (int j = 0; j < nq; ++j)
        SSW_HIP_TRY(hipMemcpyAsync(out_slabs_host + (size_t)j * idx->n, chunk_slab(idx, nq, j), (size_t)idx->n * sizeof(float),
                                   hipMemcpyDeviceToHost, idx->stream));
    SSW_TRY(do_scan(idx, idx->batch.qb_dev + (size_t)(nq - 1) * dim));  // the buffer held the sentinel
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    *out_waves = rescore_survivors_waves(idx->device, cap);
    return SSW_OK;
}

// ---- the packed 6-bit shadow of single queries (prune.hip, "6-bit shadow"; tests/test_prune6_gpu.py) ----------------
static ssw_status require_shadow6(ssw_index *idx, const char *who) {
    SSW_REQUIRE(prune6_eligible(idx), "the index takes no 6-bit shadow (ssw_tune_prune6, rows, dim, borrowed or escaped rows)");
    return require_shadow(idx, who, SHADOW_Q6);
}

ssw_status ssw_debug_prune6_shadow(ssw_index *idx, int64_t first_row, int64_t n_rows, int8_t *out_codes, float *out_scale,
                                   float *out_err) {
    SSW_REQUIRE(idx != nullptr, "idx is NULL");
    SSW_REQUIRE(first_row >= 0 && n_rows >= 0 && first_row + n_rows <= idx->n, "rows [%lld, +%lld) outside [0, %lld)",
                (long long)first_row, (long long)n_rows, (long long)idx->n);
    DeviceGuard guard(idx->device);
    SSW_TRY(require_shadow6(idx, "prune6_shadow"));
    if (n_rows == 0) return SSW_OK;
    const Shadow &s = idx->prune.sh[SHADOW_Q6];
    const int dim = idx->dim;
    const size_t tile_bytes = (size_t)16 * dim * 3 / 4;
    const int64_t tile0 = first_row >> 4, tile1 = (first_row + n_rows - 1) >> 4;
    std::vector<unsigned char> packed(out_codes ? (size_t)(tile1 - tile0 + 1) * tile_bytes : 0);
    if (out_codes)
        SSW_HIP_TRY(hipMemcpyAsync(packed.data(), s.codes + (size_t)tile0 * tile_bytes, packed.size(), hipMemcpyDeviceToHost,
                                   idx->stream));
    if (out_scale)
        SSW_HIP_TRY(hipMemcpyAsync(out_scale, s.scale + first_row, (size_t)n_rows * sizeof(float), hipMemcpyDeviceToHost,
                                   idx->stream));
    if (out_err)
        SSW_HIP_TRY(hipMemcpyAsync(out_err, s.err + first_row, (size_t)n_rows * sizeof(float), hipMemcpyDeviceToHost,
                                   idx->stream));
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    if (!out_codes) return SSW_OK;
    for (int64_t r = first_row; r < first_row + n_rows; ++r) {
        const unsigned char *tile = packed.data() + (size_t)((r >> 4) - tile0) * tile_bytes;
        for (int i = 0; i < dim; ++i) {
            int u, g, j;
            q6_slot(i, &u, &g, &j);
            const int lane = 16 * g + (int)(r & 15);
            int c;
            if (j < 12) {
                c = (int8_t)tile[q6_word_offset(lane, 3 * u + j / 4) + (size_t)(j % 4)] >> 2;  // arithmetic: sign kept
            } else {
                unsigned bits = 0u;
                for (int part = 0; part < 3; ++part)
                    bits = (bits << 2) | (tile[q6_word_offset(lane, 3 * u + part) + (size_t)(j - 12)] & 3u);
                c = (int)(bits ^ 32u) - 32;  // six bits, two's complement
            }
            out_codes[(size_t)(r - first_row) * dim + i] = (int8_t)c;
        }
    }
    return SSW_OK;
}

ssw_status ssw_debug_prune6_bounds(ssw_index *idx, const float *q_host, int64_t *out_I, float *out_lb, float *out_Qe,
                                   int8_t *out_codes) {
    SSW_REQUIRE(idx != nullptr && q_host != nullptr, "NULL argument");
    DeviceGuard guard(idx->device);
    SSW_TRY(require_shadow6(idx, "prune6_bounds"));
    PruneState &p = idx->prune;
    const size_t dim = (size_t)idx->dim;
    int64_t *dbg = nullptr;
    if (out_I) SSW_HIP_TRY(hipMalloc((void **)&dbg, (size_t)idx->n * sizeof(int64_t)));
    unsigned st[Q8_MQ_WORDS] = {};
    std::vector<int8_t> planes(q6_plane_bytes(idx->dim));
    auto run = [&]() -> ssw_status {
        SSW_TRY(idx->q_stage.push(idx->q_dev, q_host, dim * sizeof(float), idx->stream));
        SSW_TRY(prune_bounds(idx, SHADOW_Q6, idx->q_dev, dbg));  // as in scan_for_topk: readers complete the buffer with q_last
        if (out_I) SSW_HIP_TRY(hipMemcpyAsync(out_I, dbg, (size_t)idx->n * sizeof(int64_t), hipMemcpyDeviceToHost, idx->stream));
        if (out_lb)
            SSW_HIP_TRY(hipMemcpyAsync(out_lb, idx->scores, (size_t)idx->n * sizeof(float), hipMemcpyDeviceToHost, idx->stream));
        SSW_HIP_TRY(hipMemcpyAsync(st, p.state6, sizeof(st), hipMemcpyDeviceToHost, idx->stream));
        SSW_HIP_TRY(hipMemcpyAsync(planes.data(), p.planes6, planes.size(), hipMemcpyDeviceToHost, idx->stream));
        SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
        return SSW_OK;
    };
    const ssw_status rc = run();
    if (rc != SSW_OK) (void)hipStreamSynchronize(idx->stream);
    (void)hipFree(dbg);
    SSW_TRY(rc);
    if (out_Qe) {
        memcpy(out_Qe, &st[1], 4);      // Q
        memcpy(out_Qe + 1, &st[3], 4);  // e
        memcpy(out_Qe + 2, &st[4], 4);  // t2
        out_Qe[3] = (float)st[2];       // 1 = the query cannot be bounded
    }
    if (out_codes)  // the operand's columns 0 (hi) and 1 (lo) back to natural element order
        for (int pl = 0; pl < 2; ++pl)
            for (size_t i = 0; i < dim; ++i) {
                int u, g, j;
                q6_slot((int)i, &u, &g, &j);
                out_codes[(size_t)pl * dim + i] = planes[(size_t)(u * 64 + g * 16 + pl) * 16 + (size_t)j];
            }
    return SSW_OK;
}

// ---- the survivor pass's pre-test (tests/test_prune_tail_gpu.py) ------------------------------------------------------
ssw_status ssw_debug_prune_maxima(ssw_index *idx, int32_t six, float *out2) {
    SSW_REQUIRE(idx != nullptr && out2 != nullptr, "NULL argument");
    DeviceGuard guard(idx->device);
    if (six) SSW_TRY(require_shadow6(idx, "prune_maxima"));
    else {
        SSW_REQUIRE(prune_eligible(idx), "the index is not pruned (ssw_tune_prune, dim, borrowed or escaped rows)");
        SSW_TRY(require_shadow(idx, "prune_maxima"));
    }
    SSW_HIP_TRY(hipMemcpyAsync(out2, idx->prune.sh[six ? SHADOW_Q6 : SHADOW_Q8].max, SHADOW_MAX_WORDS * sizeof(float),
                               hipMemcpyDeviceToHost, idx->stream));
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    return SSW_OK;
}

ssw_status ssw_debug_prune6_survivors(ssw_index *idx, float threshold, int32_t k, int32_t sel_count, int32_t sel_overflow,
                                      int64_t cap, int32_t *out_published, int64_t *out_collected, int64_t *out_rows) {
    SSW_REQUIRE(idx != nullptr && out_published != nullptr && out_collected != nullptr, "NULL argument");
    SSW_REQUIRE(k >= 1 && k <= SSW_MAX_TOPK, "k=%d outside [1, %d]", k, SSW_MAX_TOPK);
    SSW_REQUIRE(cap >= 0 && cap <= SURV_CAP, "cap=%lld outside [0, %lld]", (long long)cap, (long long)SURV_CAP);
    SSW_REQUIRE(cap == 0 || out_rows != nullptr, "out_rows is NULL");
    SSW_REQUIRE(idx->scores_partial && shadow_current(idx, SHADOW_Q6), "no bounds in the buffer: ssw_debug_prune6_bounds first");
    DeviceGuard guard(idx->device);
    SSW_TRY(ensure_ws(idx));
    unsigned *st = idx->prune.state6;
    SSW_HIP_TRY(hipMemsetAsync(st, 0, sizeof(unsigned), idx->stream));      // the counter and the "selection failed"
    SSW_HIP_TRY(hipMemsetAsync(st + 5, 0, sizeof(unsigned), idx->stream));  // word k_q6_query resets
    SSW_TRY(stand_in_threshold(idx, threshold, k, sel_count, sel_overflow));
    int32_t m = -1;
    SSW_TRY(prune_survivors(idx, SHADOW_Q6, k, cap, nullptr, &m));
    unsigned collected = 0u;
    SSW_HIP_TRY(hipMemcpyAsync(&collected, st, sizeof(unsigned), hipMemcpyDeviceToHost, idx->stream));
    if (m > 0)
        SSW_HIP_TRY(hipMemcpyAsync(out_rows, idx->prune.surv_rows, (size_t)m * sizeof(int64_t), hipMemcpyDeviceToHost,
                                   idx->stream));
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    *out_published = m;
    *out_collected = (int64_t)collected;
    return SSW_OK;
}

// ---- the pruned batch's chunk on the 6-bit shadow (prune.hip, k_q6_query_mq / k_q6_bounds_mq; tests/test_prune6_batch_gpu.py)
ssw_status ssw_debug_prune6_scan_mq_shape(ssw_index *idx, int32_t *out_blocks, int32_t *out_tiles) {
    SSW_REQUIRE(idx != nullptr && out_blocks != nullptr && out_tiles != nullptr, "NULL argument");
    SSW_REQUIRE(q6_dim_supported(idx->dim), "dim=%d has no shadow scan", idx->dim);
    int blocks = 0, tiles = 0;
    scan_shape(SCAN_Q6_MQ, idx->dim, idx->device, idx->n, &blocks, &tiles);
    *out_blocks = blocks;
    *out_tiles = tiles;
    return SSW_OK;
}

ssw_status ssw_debug_prune6_bounds_mq(ssw_index *idx, const float *q_host, int32_t nq, int64_t *out_I, float *out_lb,
                                      float *out_Qe, int8_t *out_codes) {
    SSW_REQUIRE(idx != nullptr && q_host != nullptr, "NULL argument");
    SSW_REQUIRE(nq >= 1 && nq <= Q8_MQ_WIDTH, "nq=%d outside [1, %d]", nq, Q8_MQ_WIDTH);
    DeviceGuard guard(idx->device);
    SSW_TRY(debug_chunk_ready(idx, nq, true));
    PruneBatchState &pb = idx->prune_batch;
    const size_t dim = (size_t)idx->dim, cells = (size_t)nq * idx->n;
    int64_t *dbg = nullptr;
    if (out_I) SSW_HIP_TRY(hipMalloc((void **)&dbg, cells * sizeof(int64_t)));
    std::vector<unsigned> mq((size_t)Q8_MQ_WIDTH * Q8_MQ_WORDS);
    std::vector<int8_t> planes(q8_mq_plane_bytes(idx->dim));
    auto run = [&]() -> ssw_status {
        SSW_TRY(idx->batch.qb_stage.push(idx->batch.qb_dev, q_host, (size_t)nq * dim * sizeof(float), idx->stream));
        SSW_TRY(prune_bounds_mq(idx, nq, nullptr, nullptr, dbg));
        if (out_I) SSW_HIP_TRY(hipMemcpyAsync(out_I, dbg, cells * sizeof(int64_t), hipMemcpyDeviceToHost, idx->stream));
        if (out_lb)
            for (int j = 0; j < nq; ++j)
                SSW_HIP_TRY(hipMemcpyAsync(out_lb + (size_t)j * idx->n, chunk_slab(idx, nq, j), (size_t)idx->n * sizeof(float),
                                           hipMemcpyDeviceToHost, idx->stream));
        SSW_HIP_TRY(hipMemcpyAsync(mq.data(), pb.mq, mq.size() * sizeof(unsigned), hipMemcpyDeviceToHost, idx->stream));
        SSW_HIP_TRY(hipMemcpyAsync(planes.data(), pb.planes, planes.size(), hipMemcpyDeviceToHost, idx->stream));
        SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
        return SSW_OK;
    };
    const ssw_status st = run();
    if (st != SSW_OK) (void)hipStreamSynchronize(idx->stream);
    (void)hipFree(dbg);
    SSW_TRY(st);
    for (int b = 0; b < nq; ++b) {
        const unsigned *w = mq.data() + (size_t)b * Q8_MQ_WORDS;
        if (out_Qe) {
            memcpy(out_Qe + 4 * b, &w[1], 4);      // Q
            memcpy(out_Qe + 4 * b + 1, &w[3], 4);  // e
            memcpy(out_Qe + 4 * b + 2, &w[4], 4);  // t2
            out_Qe[4 * b + 3] = (float)w[2];       // 1 = the query cannot be bounded
        }
        if (out_codes)  // the operand's placement (q6_slot) back to natural element order
            for (int pl = 0; pl < 2; ++pl)
                for (size_t i = 0; i < dim; ++i) {
                    int u, g, j;
                    q6_slot((int)i, &u, &g, &j);
                    out_codes[((size_t)b * 2 + pl) * dim + i] = planes[(size_t)((u * 2 + pl) * 64 + 16 * g + b) * 16 + (size_t)j];
                }
    }
    return SSW_OK;
}

ssw_status ssw_debug_prune6_survivors_mq(ssw_index *idx, int32_t nq, int32_t slot, float threshold, int32_t k,
                                         int32_t sel_count, int32_t sel_overflow, int64_t cap, int32_t *out_published,
                                         int64_t *out_collected, int64_t *out_rows) {
    SSW_REQUIRE(idx != nullptr && out_published != nullptr && out_collected != nullptr, "NULL argument");
    SSW_REQUIRE(nq >= 1 && nq <= Q8_MQ_WIDTH && slot >= 0 && slot < nq, "slot=%d outside the chunk of %d", slot, nq);
    SSW_REQUIRE(k >= 1 && k <= SSW_MAX_TOPK, "k=%d outside [1, %d]", k, SSW_MAX_TOPK);
    SSW_REQUIRE(cap >= 0 && cap <= SURV_CAP, "cap=%lld outside [0, %lld]", (long long)cap, (long long)SURV_CAP);
    SSW_REQUIRE(cap == 0 || out_rows != nullptr, "out_rows is NULL");
    PruneBatchState &pb = idx->prune_batch;
    SSW_REQUIRE(idx->scores_partial && pb.kind == SHADOW_Q6 && shadow_current(idx, SHADOW_Q6) && pb.slots >= nq &&
                    idx->batch.side_slabs >= nq - 1,
                "no bounds of such a chunk in the buffers: ssw_debug_prune6_bounds_mq first");
    DeviceGuard guard(idx->device);
    SSW_TRY(ensure_ws(idx));
    unsigned *st = pb.mq + slot * Q8_MQ_WORDS;
    SSW_HIP_TRY(hipMemsetAsync(st, 0, sizeof(unsigned), idx->stream));      // the counter and the "selection failed"
    SSW_HIP_TRY(hipMemsetAsync(st + 5, 0, sizeof(unsigned), idx->stream));  // word k_q6_query_mq resets
    SSW_TRY(stand_in_threshold(idx, threshold, k, sel_count, sel_overflow));
    SSW_TRY(prune_survivors_slot(idx, nq, slot, k, cap));
    int32_t m[Q8_MQ_WIDTH];
    SSW_TRY(prune_publish_mq(idx, nq, cap, nullptr, m));
    unsigned collected = 0u;
    SSW_HIP_TRY(hipMemcpyAsync(&collected, st, sizeof(unsigned), hipMemcpyDeviceToHost, idx->stream));
    if (m[slot] > 0)
        SSW_HIP_TRY(hipMemcpyAsync(out_rows, pb.surv_rows + (int64_t)slot * SURV_CAP, (size_t)m[slot] * sizeof(int64_t),
                                   hipMemcpyDeviceToHost, idx->stream));
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    *out_published = m[slot];
    *out_collected = (int64_t)collected;
    return SSW_OK;
}

// ---- the packed 5-bit shadow of single queries (prune.hip, "5-bit shadow"; tests/test_prune5_gpu.py) ----------------
static ssw_status require_shadow5(ssw_index *idx, const char *who) {
    SSW_REQUIRE(prune5_eligible(idx),
                "the index takes no 5-bit shadow (ssw_tune_prune5, rows, dim, dtype, image map, borrowed or escaped rows)");
    return require_shadow(idx, who, SHADOW_Q5);
}

ssw_status ssw_debug_prune5_scan_shape(ssw_index *idx, int32_t *out_blocks, int32_t *out_tiles) {
    SSW_REQUIRE(idx != nullptr && out_blocks != nullptr && out_tiles != nullptr, "NULL argument");
    SSW_REQUIRE(q5_dim_supported(idx->dim), "dim=%d has no 5-bit shadow scan", idx->dim);
    int blocks = 0, tiles = 0;
    scan_shape(SCAN_Q5, idx->dim, idx->device, idx->n, &blocks, &tiles);
    *out_blocks = blocks;
    *out_tiles = tiles;
    return SSW_OK;
}

ssw_status ssw_debug_prune5_shadow(ssw_index *idx, int64_t first_row, int64_t n_rows, int8_t *out_codes, float *out_scale,
                                   float *out_err) {
    SSW_REQUIRE(idx != nullptr, "idx is NULL");
    SSW_REQUIRE(first_row >= 0 && n_rows >= 0 && first_row + n_rows <= idx->n, "rows [%lld, +%lld) outside [0, %lld)",
                (long long)first_row, (long long)n_rows, (long long)idx->n);
    DeviceGuard guard(idx->device);
    SSW_TRY(require_shadow5(idx, "prune5_shadow"));
    if (n_rows == 0) return SSW_OK;
    const Shadow &s = idx->prune.sh[SHADOW_Q5];
    const int dim = idx->dim;
    const size_t tile_bytes = (size_t)16 * dim * 5 / 8;
    const int64_t tile0 = first_row >> 4, tile1 = (first_row + n_rows - 1) >> 4;
    std::vector<unsigned char> packed(out_codes ? (size_t)(tile1 - tile0 + 1) * tile_bytes : 0);
    if (out_codes)
        SSW_HIP_TRY(hipMemcpyAsync(packed.data(), s.codes + (size_t)tile0 * tile_bytes, packed.size(), hipMemcpyDeviceToHost,
                                   idx->stream));
    if (out_scale)
        SSW_HIP_TRY(hipMemcpyAsync(out_scale, s.scale + first_row, (size_t)n_rows * sizeof(float), hipMemcpyDeviceToHost,
                                   idx->stream));
    if (out_err)
        SSW_HIP_TRY(hipMemcpyAsync(out_err, s.err + first_row, (size_t)n_rows * sizeof(float), hipMemcpyDeviceToHost,
                                   idx->stream));
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    if (!out_codes) return SSW_OK;
    for (int64_t r = first_row; r < first_row + n_rows; ++r) {
        const unsigned char *tile = packed.data() + (size_t)((r >> 4) - tile0) * tile_bytes;
        for (int i = 0; i < dim; ++i) {
            int u, g, j;
            q6_slot(i, &u, &g, &j);
            const int lane = 16 * g + (int)(r & 15);
            Q5Field f[3];
            const int nf = q5_fields(u, j, f);
            unsigned bits = 0u;
            for (int t = 0; t < nf; ++t)
                bits |= ((tile[q6_word_offset(lane, f[t].word) + (size_t)f[t].byte] >> f[t].lo) & ((1u << f[t].bits) - 1u)) << f[t].from;
            out_codes[(size_t)(r - first_row) * dim + i] = (int8_t)((int)(bits ^ 16u) - 16);  // five bits, two's complement
        }
    }
    return SSW_OK;
}

ssw_status ssw_debug_prune5_bounds(ssw_index *idx, const float *q_host, int64_t *out_I, float *out_lb, float *out_Qe,
                                   int8_t *out_codes) {
    SSW_REQUIRE(idx != nullptr && q_host != nullptr, "NULL argument");
    DeviceGuard guard(idx->device);
    SSW_TRY(require_shadow5(idx, "prune5_bounds"));
    PruneState &p = idx->prune;
    const size_t dim = (size_t)idx->dim;
    int64_t *dbg = nullptr;
    if (out_I) SSW_HIP_TRY(hipMalloc((void **)&dbg, (size_t)idx->n * sizeof(int64_t)));
    unsigned st[Q8_MQ_WORDS] = {};
    std::vector<int8_t> planes(q6_plane_bytes(idx->dim));
    auto run = [&]() -> ssw_status {
        SSW_TRY(idx->q_stage.push(idx->q_dev, q_host, dim * sizeof(float), idx->stream));
        SSW_TRY(prune_bounds(idx, SHADOW_Q5, idx->q_dev, dbg));  // as in scan_for_topk: readers complete the buffer with q_last
        if (out_I) SSW_HIP_TRY(hipMemcpyAsync(out_I, dbg, (size_t)idx->n * sizeof(int64_t), hipMemcpyDeviceToHost, idx->stream));
        if (out_lb)
            SSW_HIP_TRY(hipMemcpyAsync(out_lb, idx->scores, (size_t)idx->n * sizeof(float), hipMemcpyDeviceToHost, idx->stream));
        SSW_HIP_TRY(hipMemcpyAsync(st, p.state6, sizeof(st), hipMemcpyDeviceToHost, idx->stream));
        SSW_HIP_TRY(hipMemcpyAsync(planes.data(), p.planes6, planes.size(), hipMemcpyDeviceToHost, idx->stream));
        SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
        return SSW_OK;
    };
    const ssw_status rc = run();
    if (rc != SSW_OK) (void)hipStreamSynchronize(idx->stream);
    (void)hipFree(dbg);
    SSW_TRY(rc);
    if (out_Qe) {
        memcpy(out_Qe, &st[1], 4);      // Q
        memcpy(out_Qe + 1, &st[3], 4);  // e
        memcpy(out_Qe + 2, &st[4], 4);  // t2
        out_Qe[3] = (float)st[2];       // 1 = the query cannot be bounded
    }
    if (out_codes)  // the operand's columns 0 (hi) and 1 (lo) back to natural element order
        for (int pl = 0; pl < 2; ++pl)
            for (size_t i = 0; i < dim; ++i) {
                int u, g, j;
                q6_slot((int)i, &u, &g, &j);
                out_codes[(size_t)pl * dim + i] = planes[(size_t)(u * 64 + g * 16 + pl) * 16 + (size_t)j];
            }
    return SSW_OK;
}

ssw_status ssw_debug_prune5_survivors(ssw_index *idx, float threshold, int32_t k, int32_t sel_count, int32_t sel_overflow,
                                      int64_t cap, int32_t *out_published, int64_t *out_collected, int64_t *out_rows) {
    SSW_REQUIRE(idx != nullptr && out_published != nullptr && out_collected != nullptr, "NULL argument");
    SSW_REQUIRE(k >= 1 && k <= SSW_MAX_TOPK, "k=%d outside [1, %d]", k, SSW_MAX_TOPK);
    SSW_REQUIRE(cap >= 0 && cap <= SURV_CAP, "cap=%lld outside [0, %lld]", (long long)cap, (long long)SURV_CAP);
    SSW_REQUIRE(cap == 0 || out_rows != nullptr, "out_rows is NULL");
    SSW_REQUIRE(idx->scores_partial && shadow_current(idx, SHADOW_Q5), "no bounds in the buffer: ssw_debug_prune5_bounds first");
    DeviceGuard guard(idx->device);
    SSW_TRY(ensure_ws(idx));
    unsigned *st = idx->prune.state6;
    SSW_HIP_TRY(hipMemsetAsync(st, 0, sizeof(unsigned), idx->stream));      // the counter and the "selection failed"
    SSW_HIP_TRY(hipMemsetAsync(st + 5, 0, sizeof(unsigned), idx->stream));  // word k_q6_query resets
    SSW_TRY(stand_in_threshold(idx, threshold, k, sel_count, sel_overflow));
    int32_t m = -1;
    SSW_TRY(prune_survivors(idx, SHADOW_Q5, k, cap, nullptr, &m));
    unsigned collected = 0u;
    SSW_HIP_TRY(hipMemcpyAsync(&collected, st, sizeof(unsigned), hipMemcpyDeviceToHost, idx->stream));
    if (m > 0)
        SSW_HIP_TRY(hipMemcpyAsync(out_rows, idx->prune.surv_rows, (size_t)m * sizeof(int64_t), hipMemcpyDeviceToHost,
                                   idx->stream));
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    *out_published = m;
    *out_collected = (int64_t)collected;
    return SSW_OK;
}

// ---- the two-stage 4 + 1-bit shadow (prune.hip, "two-stage 4 + 1-bit shadow"; tests/test_prune41_gpu.py) -------------
static ssw_status require_shadow41(ssw_index *idx, const char *who) {
    SSW_REQUIRE(prune41_eligible(idx),
                "the index takes no two-stage shadow (ssw_tune_prune41, rows, dim, dtype, image map, borrowed or escaped rows)");
    return require_shadow(idx, who, SHADOW_Q41);
}

ssw_status ssw_debug_prune41_scan_shape(ssw_index *idx, int32_t *out_blocks, int32_t *out_tiles) {
    SSW_REQUIRE(idx != nullptr && out_blocks != nullptr && out_tiles != nullptr, "NULL argument");
    SSW_REQUIRE(q5_dim_supported(idx->dim), "dim=%d has no two-stage shadow scan", idx->dim);
    int blocks = 0, tiles = 0;
    scan_shape(SCAN_Q4, idx->dim, idx->device, idx->n, &blocks, &tiles);
    *out_blocks = blocks;
    *out_tiles = tiles;
    return SSW_OK;
}

ssw_status ssw_debug_prune41_shadow(ssw_index *idx, int64_t first_row, int64_t n_rows, uint8_t *out_h, uint32_t *out_fine,
                                    float *out_s5, float *out_a5, float *out_a4) {
    SSW_REQUIRE(idx != nullptr, "idx is NULL");
    SSW_REQUIRE(first_row >= 0 && n_rows >= 0 && first_row + n_rows <= idx->n, "rows [%lld, +%lld) outside [0, %lld)",
                (long long)first_row, (long long)n_rows, (long long)idx->n);
    DeviceGuard guard(idx->device);
    SSW_TRY(require_shadow41(idx, "prune41_shadow"));
    if (n_rows == 0) return SSW_OK;
    const Shadow &s = idx->prune.sh[SHADOW_Q41];
    const int dim = idx->dim;
    const size_t tile_bytes = (size_t)16 * dim / 2, fw = (size_t)dim / 32;
    const int64_t tile0 = first_row >> 4, tile1 = (first_row + n_rows - 1) >> 4;
    std::vector<unsigned char> packed(out_h ? (size_t)(tile1 - tile0 + 1) * tile_bytes : 0);
    if (out_h)
        SSW_HIP_TRY(hipMemcpyAsync(packed.data(), s.codes + (size_t)tile0 * tile_bytes, packed.size(), hipMemcpyDeviceToHost,
                                   idx->stream));
    if (out_fine)
        SSW_HIP_TRY(hipMemcpyAsync(out_fine, s.fine + (size_t)first_row * fw, (size_t)n_rows * fw * sizeof(uint32_t),
                                   hipMemcpyDeviceToHost, idx->stream));
    const float *src[3] = {s.scale, s.err, s.err4};
    float *dst[3] = {out_s5, out_a5, out_a4};
    for (int t = 0; t < 3; ++t)
        if (dst[t])
            SSW_HIP_TRY(hipMemcpyAsync(dst[t], src[t] + first_row, (size_t)n_rows * sizeof(float), hipMemcpyDeviceToHost,
                                       idx->stream));
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    if (!out_h) return SSW_OK;
    for (int64_t r = first_row; r < first_row + n_rows; ++r) {
        const unsigned char *tile = packed.data() + (size_t)((r >> 4) - tile0) * tile_bytes;
        for (int i = 0; i < dim; ++i) {
            int u, g, j, word, byte, shift;
            q6_slot(i, &u, &g, &j);
            q4_nibble(u, j, &word, &byte, &shift);
            out_h[(size_t)(r - first_row) * dim + i] =
                (uint8_t)((tile[q6_word_offset(16 * g + (int)(r & 15), word) + (size_t)byte] >> shift) & 15u);
        }
    }
    return SSW_OK;
}

ssw_status ssw_debug_prune41_stage1(ssw_index *idx, const float *q_host, int32_t *out_H, float *out_lb4, float *out_Qe,
                                    int32_t *out_sumD) {
    SSW_REQUIRE(idx != nullptr && q_host != nullptr, "NULL argument");
    DeviceGuard guard(idx->device);
    SSW_TRY(require_shadow41(idx, "prune41_stage1"));
    PruneState &p = idx->prune;
    unsigned st[Q8_MQ_WORDS] = {};
    SSW_TRY(idx->q_stage.push(idx->q_dev, q_host, (size_t)idx->dim * sizeof(float), idx->stream));
    SSW_TRY(prune_bounds(idx, SHADOW_Q41, idx->q_dev, nullptr));  // as in scan_for_topk: readers complete the buffer with q_last
    if (out_H)
        SSW_HIP_TRY(hipMemcpyAsync(out_H, p.sh[SHADOW_Q41].H, (size_t)idx->n * sizeof(int32_t), hipMemcpyDeviceToHost, idx->stream));
    if (out_lb4)
        SSW_HIP_TRY(hipMemcpyAsync(out_lb4, idx->scores, (size_t)idx->n * sizeof(float), hipMemcpyDeviceToHost, idx->stream));
    SSW_HIP_TRY(hipMemcpyAsync(st, p.state6, sizeof(st), hipMemcpyDeviceToHost, idx->stream));
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    if (out_Qe) {
        memcpy(out_Qe, &st[1], 4);      // Q
        memcpy(out_Qe + 1, &st[3], 4);  // e
        memcpy(out_Qe + 2, &st[4], 4);  // t2
        out_Qe[3] = (float)st[2];       // 1 = the query cannot be bounded
    }
    if (out_sumD) out_sumD[0] = (int32_t)st[6], out_sumD[1] = (int32_t)st[7];
    return SSW_OK;
}

// the counters the two stages add to, and the "selection failed" word, as k_q41_query leaves them
static ssw_status reset_stage_words(ssw_index *idx) {
    unsigned *st = idx->prune.state6;
    SSW_HIP_TRY(hipMemsetAsync(st, 0, sizeof(unsigned), idx->stream));
    SSW_HIP_TRY(hipMemsetAsync(st + 5, 0, sizeof(unsigned), idx->stream));
    SSW_HIP_TRY(hipMemsetAsync(idx->prune.cstate, 0, Q41_STATE_WORDS * sizeof(unsigned), idx->stream));
    return SSW_OK;
}

ssw_status ssw_debug_prune41_survivors1(ssw_index *idx, float threshold, int32_t k, int32_t blocks, int64_t rows_cap,
                                        int64_t *out_count, uint32_t *out_rows) {
    SSW_REQUIRE(idx != nullptr && out_count != nullptr, "NULL argument");
    SSW_REQUIRE(k >= 1 && k <= SSW_MAX_TOPK, "k=%d outside [1, %d]", k, SSW_MAX_TOPK);
    SSW_REQUIRE(blocks >= 0 && blocks <= 65536, "blocks=%d outside [0, 65536]", blocks);
    SSW_REQUIRE(rows_cap >= 0 && (rows_cap == 0 || out_rows != nullptr), "out_rows is NULL");
    SSW_REQUIRE(idx->scores_partial && shadow_current(idx, SHADOW_Q41), "no bounds in the buffer: ssw_debug_prune41_stage1 first");
    DeviceGuard guard(idx->device);
    SSW_TRY(ensure_ws(idx));
    SSW_TRY(reset_stage_words(idx));
    SSW_TRY(stand_in_threshold(idx, threshold, k, k, 0));
    SSW_TRY(prune41_stage1(idx, k, blocks));
    unsigned count = 0u;
    SSW_HIP_TRY(hipMemcpyAsync(&count, idx->prune.cstate, sizeof(unsigned), hipMemcpyDeviceToHost, idx->stream));
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    const int64_t m = std::min<int64_t>(std::min<int64_t>(count, COARSE_CAP), rows_cap);
    if (m > 0) SSW_HIP_TRY(hipMemcpy(out_rows, idx->prune.coarse_rows, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost));
    *out_count = (int64_t)count;
    return SSW_OK;
}

ssw_status ssw_debug_prune41_refine(ssw_index *idx, const uint32_t *rows, int64_t m, float threshold, int32_t k,
                                    float *out_lb5, int32_t *out_B, int64_t *out_survivors, int64_t *out_surv_rows) {
    SSW_REQUIRE(idx != nullptr && out_lb5 != nullptr && out_B != nullptr && out_survivors != nullptr, "NULL argument");
    SSW_REQUIRE(k >= 1 && k <= SSW_MAX_TOPK, "k=%d outside [1, %d]", k, SSW_MAX_TOPK);
    SSW_REQUIRE(m >= 0 && m <= COARSE_CAP && (m == 0 || rows != nullptr), "m=%lld outside [0, %lld]", (long long)m, (long long)COARSE_CAP);
    SSW_REQUIRE(idx->scores_partial && shadow_current(idx, SHADOW_Q41), "no bounds in the buffer: ssw_debug_prune41_stage1 first");
    DeviceGuard guard(idx->device);
    SSW_TRY(ensure_ws(idx));
    PruneState &p = idx->prune;
    const bool dense = m > prune41_coarse_cap();
    const int64_t entries = dense ? idx->n : m;
    float *lb5 = nullptr;
    int32_t *B = nullptr;
    auto run = [&]() -> ssw_status {
        SSW_HIP_TRY(hipMalloc((void **)&lb5, (size_t)std::max<int64_t>(entries, 1) * sizeof(float)));
        SSW_HIP_TRY(hipMalloc((void **)&B, (size_t)std::max<int64_t>(entries, 1) * sizeof(int32_t)));
        SSW_TRY(reset_stage_words(idx));
        SSW_TRY(stand_in_threshold(idx, threshold, k, k, 0));
        const unsigned count = (unsigned)m;
        if (m > 0) SSW_HIP_TRY(hipMemcpy(p.coarse_rows, rows, (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice));
        SSW_HIP_TRY(hipMemcpy(p.cstate, &count, sizeof(unsigned), hipMemcpyHostToDevice));
        SSW_TRY(prune41_refine(idx, k, nullptr, SURV_CAP, lb5, B));
        unsigned found = 0u;
        SSW_HIP_TRY(hipMemcpyAsync(&found, p.state6, sizeof(unsigned), hipMemcpyDeviceToHost, idx->stream));
        SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
        if (entries > 0) {
            SSW_HIP_TRY(hipMemcpy(out_lb5, lb5, (size_t)entries * sizeof(float), hipMemcpyDeviceToHost));
            SSW_HIP_TRY(hipMemcpy(out_B, B, (size_t)entries * sizeof(int32_t), hipMemcpyDeviceToHost));
        }
        const int64_t got = std::min<int64_t>(found, SURV_CAP);
        if (got > 0 && out_surv_rows)
            SSW_HIP_TRY(hipMemcpy(out_surv_rows, p.surv_rows, (size_t)got * sizeof(int64_t), hipMemcpyDeviceToHost));
        *out_survivors = (int64_t)found;
        return SSW_OK;
    };
    const ssw_status rc = run();
    if (rc != SSW_OK) (void)hipStreamSynchronize(idx->stream);
    (void)hipFree(lb5);
    (void)hipFree(B);
    return rc;
}

ssw_status ssw_debug_prune6_scan_shape(ssw_index *idx, int32_t *out_blocks, int32_t *out_tiles) {
    SSW_REQUIRE(idx != nullptr && out_blocks != nullptr && out_tiles != nullptr, "NULL argument");
    SSW_REQUIRE(q6_dim_supported(idx->dim), "dim=%d has no shadow scan", idx->dim);
    int blocks = 0, tiles = 0;
    scan_shape(SCAN_Q6, idx->dim, idx->device, idx->n, &blocks, &tiles);
    *out_blocks = blocks;
    *out_tiles = tiles;
    return SSW_OK;
}

// The f64 loss of the engine's last one-output evaluation (fb_eval leaves it in loss_host[0]; ssw_fb_lossgrad hands out
// its f32 rounding, the fit drivers compare this value).  Host code only: fb_handle.h is included for the handle's
// layout, none of fb_math.h's arithmetic is instantiated here.
ssw_status ssw_debug_fb_last_loss(const ssw_fb *fb, double *out) {
    SSW_REQUIRE(fb != nullptr && out != nullptr, "NULL argument");
    *out = fb->loss_host[0];
    return SSW_OK;
}

}  // extern "C"
