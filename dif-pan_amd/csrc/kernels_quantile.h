// Per-sample quantile of |v| for dynamic thresholding (Imagen; diffusion_ddpm_pan.py:327-344, solver/dpm_solver.py:424-433): an EXACT order-statistic
// selection, one workgroup per sample.
//
// |v| is read as its 32-bit pattern: non-negative floats order like unsigned integers, so the k-th smallest |v| is the k-th smallest key.  Radix select
// from the most significant byte: four passes, each a 256-bin histogram in LDS of the keys that still share the selected prefix, then one wave scans the
// bins for the one that holds rank k.  Counts are integers and additions of them commute, so the result is bitwise deterministic whatever the arrival order
// of the LDS atomics, and a sample of a batch gives what the sample alone gives (one workgroup sees one sample and nothing else).
//
// torch.quantile's linear interpolation needs the order statistics of rank floor(r) and ceil(r).  The last pass leaves the count of keys EQUAL to the first
// one and its rank among them: the second is the same value while that bucket has room, else the smallest key above the first -- one min pass, no selection.
//
// n <= QUANT_RESIDENT_MAX (a 64 x 64 x 8 tile: 32 768 keys = 128 KiB of the 160 KiB LDS): the keys are computed once, kept in LDS, and every pass reads LDS.
// Larger samples (CAVE 128 x 128 x 31) recompute the key from memory in every pass.
//
// A thread walks its keys with stride blockDim.x (coalesced) and adds RUNS of equal digits with one atomic: the top byte of image-like data takes two or
// three values and a clamped image is half zeros, which would otherwise serialise a whole wave on one LDS address.
#pragma once
#include "quantile_args.h"

namespace ddif {

enum { QUANT_HDR_BYTES = 2048 };  // hist[256] | ctl[16] | wmin[16] in front of the resident keys

// model_wrapper's model_type branch (solver/dpm_solver.py:296-303) as dpm_x0_kernel evaluates it
__device__ __forceinline__ float quant_dpm_eps(const QuantArgs& a, float xv, float o) {
#pragma clang fp contract(off)
    if (a.pred == 0) return (xv - a.alpha * o) / a.sigma;
    if (a.pred == 1) return o;
    const float p = a.alpha * o, q = a.sigma * xv;
    return p + q;
}

__device__ __forceinline__ unsigned quant_key(const QuantArgs& a, size_t i, float px, float po) {
#pragma clang fp contract(off)
    float v;
    if (a.form == QUANT_RAW) {
        v = a.a[i];
    } else if (a.form == QUANT_DDPM) {  // ddpm_step_kernel up to the clamp
        float x0 = a.a[i];
        if (a.pred) x0 = pred_x0(px, a.xt[i], po, x0);
        v = x0 + a.lms[i];
    } else {  // dpm_x0_kernel up to the corrector
        const float xv = a.xt[i];
        float eps = quant_dpm_eps(a, xv, a.a[i]);
        if (a.a2) {  // the guided noise prediction of dpm_eval_update_kernel, in its operand order
            const float d = quant_dpm_eps(a, xv, a.a2[i]) - eps;
            const float gd = a.gscale * d;
            eps = eps + gd;
        }
        v = (xv - a.sigma * eps) / a.alpha;
    }
    return __builtin_bit_cast(unsigned, v) & 0x7fffffffu;
}

template <bool RES>
__global__ __launch_bounds__(1024) void quantile_abs_kernel(QuantArgs a) {
    DDIF_DYN_SMEM(smem);
    unsigned* hist = reinterpret_cast<unsigned*>(smem);
    unsigned* ctl = hist + 256;
    unsigned* wmin = ctl + 16;
    unsigned* keys = reinterpret_cast<unsigned*>(smem + QUANT_HDR_BYTES);
    const unsigned tid = threadIdx.x, T = blockDim.x;
    const unsigned n = (unsigned)a.n;
    const size_t base = (size_t)blockIdx.x * (size_t)a.n;
    float px = 0.f, po = 0.f;
    if (a.form == QUANT_DDPM && a.pred) {
        const int k = *a.step;
        px = a.run->tab[6][k];
        po = a.run->tab[7][k];
    }
    if (RES) {
        for (unsigned i = tid; i < n; i += T) keys[i] = quant_key(a, base + i, px, po);
        __syncthreads();
    }
    auto key_at = [&](unsigned i) -> unsigned { return RES ? keys[i] : quant_key(a, base + i, px, po); };

    unsigned prefix = 0, himask = 0, k = (unsigned)a.k_lo, ceq = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (unsigned j = tid; j < 256; j += T) hist[j] = 0;
        __syncthreads();
        unsigned cur = 0, cnt = 0;
        for (unsigned i = tid; i < n; i += T) {
            const unsigned key = key_at(i);
            if ((key & himask) != prefix) continue;
            const unsigned d = (key >> shift) & 255u;
            if (cnt && d == cur) {
                ++cnt;
            } else {
                if (cnt) atomicAdd(&hist[cur], cnt);
                cur = d;
                cnt = 1;
            }
        }
        if (cnt) atomicAdd(&hist[cur], cnt);
        __syncthreads();
        if (tid < 64) {  // wave 0: lane l owns bins 4l .. 4l+3; inclusive scan over the lanes, the lane whose range holds rank k picks the bin
            const unsigned c0 = hist[4 * tid], c1 = hist[4 * tid + 1], c2 = hist[4 * tid + 2], c3 = hist[4 * tid + 3];
            const unsigned t = c0 + c1 + c2 + c3;
            unsigned inc = t;
            for (unsigned d = 1; d < 64; d <<= 1) {
                const unsigned o = __shfl(inc, (int)((tid - d) & 63u));
                if (tid >= d) inc += o;
            }
            const unsigned exc = inc - t;
            if (k >= exc && k < inc) {  // exactly one lane: the ranges are disjoint and k < the count of keys under the prefix
                unsigned r = k - exc, dsel = 0, csel = c0;
                if (r >= c0) {
                    r -= c0; dsel = 1; csel = c1;
                    if (r >= c1) {
                        r -= c1; dsel = 2; csel = c2;
                        if (r >= c2) { r -= c2; dsel = 3; csel = c3; }
                    }
                }
                ctl[0] = 4 * tid + dsel;
                ctl[1] = r;
                ctl[2] = csel;
            }
        }
        __syncthreads();
        prefix |= ctl[0] << shift;
        himask |= 255u << shift;
        k = ctl[1];
        ceq = ctl[2];
    }
    // prefix = the order statistic of rank k_lo; `ceq` keys equal it and k is its rank among them
    unsigned hi = prefix;
    if (k + (unsigned)(a.k_hi - a.k_lo) >= ceq) {  // (uniform over the workgroup) rank k_hi lies above the bucket: the smallest key greater than `prefix`
        unsigned m = 0xffffffffu;
        for (unsigned i = tid; i < n; i += T) {
            const unsigned key = key_at(i);
            if (key > prefix && key < m) m = key;
        }
        for (int x = 32; x >= 1; x >>= 1) {
            const unsigned o = __shfl_xor(m, x);
            m = o < m ? o : m;
        }
        if ((tid & 63u) == 0) wmin[tid >> 6] = m;
        __syncthreads();
        hi = wmin[0];
        for (unsigned wv = 1; wv < (T >> 6); ++wv) hi = wmin[wv] < hi ? wmin[wv] : hi;
    }
    if (tid == 0) {
        // at::lerp as the CPU build evaluates it (one fused multiply-add on the side of the nearer end): w < 0.5 ? fma(w, b - a, a) : fma(w - 1, b - a, b)
        const float lo_v = __builtin_bit_cast(float, prefix), hi_v = __builtin_bit_cast(float, hi);
        const float diff = hi_v - lo_v;
        const float q = a.w < 0.5f ? __builtin_fmaf(a.w, diff, lo_v) : __builtin_fmaf(a.w - 1.0f, diff, hi_v);
        a.s_out[blockIdx.x] = fmaxf(q, a.max_val);
        if (a.stat_out) {
            a.stat_out[2 * (size_t)blockIdx.x] = lo_v;
            a.stat_out[2 * (size_t)blockIdx.x + 1] = hi_v;
        }
    }
}

// x0 <- clamp(x0, lo, s_b) / s_b with lo = -s_b (solver/dpm_solver.py:432) or 0 (diffusion_ddpm_pan.py:341-343: the reference's DDPM form keeps the lower bound 0)
__global__ void threshold_apply_kernel(const float* x, const float* s, long long n, size_t total, int symmetric, float* out) {
#pragma clang fp contract(off)
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const float sb = s[i / (size_t)n];
        out[i] = fminf(fmaxf(x[i], symmetric ? -sb : 0.f), sb) / sb;
    }
}

}  // namespace ddif
