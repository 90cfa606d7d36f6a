// Host side of the per-sample quantile kernel (kernels_quantile.h): launch helpers for the plan and the stateless entry points of include/ddif.h
// (ddif_dynamic_threshold) and include/ddif_testops.h (ddif_quantile_abs_stats).
#include <atomic>
#include <cmath>
#include "ddif_net.h"
#include "kernels_quantile.h"

namespace ddif {

// ATen quantile_compute for an fp32 input: q is an fp32 tensor, ranks = q * (n - 1) in fp32, ranks_below = trunc(ranks) (non-negative: floor),
// weights = ranks - ranks_below in fp32, ranks_above = ceil(ranks)
void quantile_rank(float ratio, long long n, long long* k_lo, long long* k_hi, float* w) {
    const float r = ratio * (float)(n - 1);
    long long lo = (long long)r, hi = (long long)std::ceil(r);
    if (lo > n - 1) lo = n - 1;  // (only past 2^24 values per sample, where fp32(n - 1) may round up)
    if (hi > n - 1) hi = n - 1;
    *k_lo = lo;
    *k_hi = hi;
    *w = r - (float)lo;
}

// hipFuncSetAttribute acts on the CURRENT device: raise the dynamic-LDS limit of the resident instantiation once per device, not once per process
// (a process that drives several GPUs would otherwise launch 130 KiB of LDS on the second one without it)
int quantile_prepare() {
    static std::atomic<bool> done[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
    if (dev < 64 && done[dev].load(std::memory_order_acquire)) return 0;
    const size_t sm = QUANT_HDR_BYTES + (size_t)QUANT_RESIDENT_MAX * sizeof(unsigned);
    DDIF_HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(quantile_abs_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm));
    if (dev < 64) done[dev].store(true, std::memory_order_release);
    return 0;
}

void quantile_launch(const QuantArgs& a, int B, hipStream_t s) {
#ifdef DDIF_EMU
    const int nthr = 256;  // (the emulator runs a workgroup's threads as fibers of one OS thread: fewer, longer fibers; the counts do not depend on it)
#else
    const int nthr = a.n > 4096 ? 1024 : 256;
#endif
    if (a.n <= QUANT_RESIDENT_MAX)
        hipLaunchKernelGGL(quantile_abs_kernel<true>, dim3(B), dim3(nthr), QUANT_HDR_BYTES + (size_t)a.n * sizeof(unsigned), s, a);
    else hipLaunchKernelGGL(quantile_abs_kernel<false>, dim3(B), dim3(nthr), (size_t)QUANT_HDR_BYTES, s, a);
}

void threshold_apply_launch(const float* x, const float* s_dev, int B, long long n, int symmetric, float* out, hipStream_t s) {
    const size_t total = (size_t)B * (size_t)n;
    size_t g = (total + 255) / 256;
    if (g > 8192) g = 8192;
    hipLaunchKernelGGL(threshold_apply_kernel, dim3((unsigned)g), dim3(256), 0, s, x, s_dev, n, total, symmetric, out);
}

static int quantile_raw(const float* x, int B, long long n, float ratio, float max_val, float* s_out, float* stat_out, hipStream_t s, const char* who) {
    if (!x || !s_out) return fail(DDIF_ERR_INVALID, "%s: NULL argument", who);
    if (B < 1 || n < 1 || n > 0x7fffffffLL) return fail(DDIF_ERR_INVALID, "%s: B=%d n=%lld (1 <= n < 2^31 values per sample)", who, B, n);
    if (!(ratio >= 0.f && ratio <= 1.f)) return fail(DDIF_ERR_INVALID, "%s: ratio %g outside [0, 1]", who, (double)ratio);
    if (!(max_val >= 0.f) || std::isinf(max_val)) return fail(DDIF_ERR_INVALID, "%s: max_val %g must be finite and >= 0", who, (double)max_val);
    if (int e = quantile_prepare()) return e;
    QuantArgs a{};
    a.a = x;
    a.n = n;
    a.form = QUANT_RAW;
    quantile_rank(ratio, n, &a.k_lo, &a.k_hi, &a.w);
    a.max_val = max_val;
    a.s_out = s_out;
    a.stat_out = stat_out;
    quantile_launch(a, B, s);
    return 0;
}

}  // namespace ddif

extern "C" {

int ddif_dynamic_threshold(const float* x, int B, int64_t n, float ratio, float max_val, int symmetric, float* out, float* s_out, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int e = ddif::quantile_raw(x, B, (long long)n, ratio, max_val, s_out, nullptr, s, "ddif_dynamic_threshold")) return e;
    if (out) ddif::threshold_apply_launch(x, s_out, B, (long long)n, symmetric ? 1 : 0, out, s);
    DDIF_HIPCHK(hipGetLastError());
    return DDIF_OK;
}

int ddif_quantile_abs_stats(const float* x, int B, int64_t n, float ratio, float* s_out, float* stats, void* stream) {
    if (!stats) return ddif::fail(DDIF_ERR_INVALID, "ddif_quantile_abs_stats: NULL argument");
    if (int e = ddif::quantile_raw(x, B, (long long)n, ratio, 0.f, s_out, stats, (hipStream_t)stream, "ddif_quantile_abs_stats")) return e;
    DDIF_HIPCHK(hipGetLastError());
    return DDIF_OK;
}

}
