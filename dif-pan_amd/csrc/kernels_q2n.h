// Q2n quality index (Q4 on four bands, Q8 on eight; Garzelli & Nencini 2009, as in the pansharpening toolbox the reference's
// utils/_metric_legacy.py:15-259 was ported from).  include/ddif.h ddif_q2n states the definition; this file is its arithmetic.
//
// The hypercomplex product (x) of the definition (the reference's onion_mult, :228-259) is bilinear, and the two block images z1, z2 are
// affine in the quantised data, so a block's index depends on the data only through
//     Sg_k = sum g_k,  Sgg_k = sum g_k^2,  Sf_k = sum f_k,  Sff_k = sum f_k^2,  X_kl = sum g_k f_l      (k, l < Cp bands, n = block^2 pixels)
// which are exact in 64-bit integers (values <= 65535, n <= 4096: X < 2^44, n X and Sg Sf < 2^57).  Integer sums do not depend on their
// order, so the index is bit-identical from run to run and from batch to batch by construction, with no fp reduction anywhere.  With
//     vg_k = n Sgg_k - Sg_k^2,  vf_k = n Sff_k - Sf_k^2,  c_kl = n X_kl - Sg_k Sf_l                    (integers: n^2 x variances / covariance)
//     rt_k = n t_k = sqrt(vg_k), or n 1e-8 where vg_k = 0;   ru_k = rt_k, or n where Sg_k = 0 (the branch without a division)
// the terms of the definition are, in exact arithmetic (a_k has mean 1; the mean of y_k is d_k + 1):
//     mean|z1|^2 - |m1|^2 = sum_k vg_k / rt_k^2          mean|z2|^2 - |m2|^2 = sum_k vf_k / ru_k^2          d_k = (Sf_k - Sg_k) / ru_k
//     |m1|^2 = Cp,  |m2|^2 = sum_k (d_k + 1)^2           mean(z1 (x) z2) - m1 (x) m2 = sum_kl e_k (x) e_l  sigma_l c_kl / (rt_k ru_l)
// (sigma_0 = 1, sigma_l = -1: the conjugate in z2).  About 60 fp64 operations per band pair, free of the cancellation that the
// pixel-wise form has between mean|z|^2 and |m|^2.
//   q2n_block_kernel<CP>  one workgroup per (image, block): 256 / CP threads per gt band accumulate the integer moments, a shuffle
//                         reduction inside each 32-lane half, 8 x (4 + CP) partials through LDS, thread 0 does the fp64 tail
//   q2n_mean_kernel       one workgroup per image: fixed-order mean of its map
#pragma once
#include "ddif_dev.h"

namespace ddif {

// e_k (x) e_l = sgn[k][l] e_idx[k][l]: the Cayley-Dickson recursion of the definition on unit vectors, evaluated by the compiler.
// (a, b)(c, d) = (a c - d' conj(b'), conj(a) d' + c b') with v' = conj(v) = (v_0, -v_1, ...) applied to the upper halves b, d.
constexpr void q2n_onion_mult(const int* x, const int* y, int* out, int n) {
    if (n == 1) {
        out[0] = x[0] * y[0];
        return;
    }
    const int L = n / 2;
    int a[4] = {}, ac[4] = {}, b[4] = {}, bc[4] = {}, c[4] = {}, dc[4] = {}, r1[4] = {}, r2[4] = {}, r3[4] = {}, r4[4] = {};
    for (int i = 0; i < L; ++i) {
        const int s = i == 0 ? 1 : -1;
        a[i] = x[i], ac[i] = s * x[i];
        b[i] = x[L + i], bc[i] = s * x[L + i];
        c[i] = y[i];
        dc[i] = s * y[L + i];
    }
    q2n_onion_mult(a, c, r1, L);
    q2n_onion_mult(dc, b, r2, L);  // conj(b') = b
    q2n_onion_mult(ac, dc, r3, L);
    q2n_onion_mult(c, bc, r4, L);
    for (int i = 0; i < L; ++i) {
        out[i] = r1[i] - r2[i];
        out[L + i] = r3[i] + r4[i];
    }
}
template <int CP>
struct Q2nTable {
    int idx[CP][CP], sgn[CP][CP];
};
template <int CP>
constexpr Q2nTable<CP> q2n_make_table() {
    Q2nTable<CP> t{};
    for (int k = 0; k < CP; ++k)
        for (int l = 0; l < CP; ++l) {
            int x[8] = {}, y[8] = {}, o[8] = {};
            x[k] = 1, y[l] = 1;
            q2n_onion_mult(x, y, o, CP);
            for (int r = 0; r < CP; ++r)
                if (o[r] != 0) t.idx[k][l] = r, t.sgn[k][l] = o[r];
        }
    return t;
}

// v = rint(min(max(x * scale, 0), 65535)): fp32 multiply, round half to even (the MATLAB original's uint16(); a NaN counts as 0)
__device__ __forceinline__ unsigned q2n_quant(float x, float scale) { return (unsigned)rintf(fminf(fmaxf(x * scale, 0.f), 65535.f)); }

#define DDIF_Q2N_SMEM (8 * 12 * sizeof(unsigned long long))

template <int CP>
__global__ __launch_bounds__(256) void q2n_block_kernel(const float* gt, const float* pred, int C, int H, int W, float scale, int block, int shift, int nx,
                                                        int ny, double* map) {
    typedef unsigned long long u64;
    typedef long long i64;
    DDIF_DYN_SMEM(smem_);
    u64* red = reinterpret_cast<u64*>(smem_);  // [8 halves of 32 lanes][NA]
    constexpr int PPK = 256 / CP, NA = 4 + CP;
    const int tid = threadIdx.x, k = tid / PPK;
    const int bi = (int)(blockIdx.x % (unsigned)nx), bj = (int)((blockIdx.x / (unsigned)nx) % (unsigned)ny), b = (int)(blockIdx.x / ((unsigned)nx * (unsigned)ny));
    const size_t plane = (size_t)H * W;
    const float* gk = gt + ((size_t)b * C + (k < C ? k : 0)) * plane;
    const float* pb = pred + (size_t)b * C * plane;
    const int n = block * block;
    u64 acc[NA];  // Sg, Sgg, Sf, Sff of band k, then X[k][0 .. CP-1]
#pragma unroll
    for (int a = 0; a < NA; ++a) acc[a] = 0;
    if (k < C) {  // a zero band appended up to CP has all-zero moments
        for (int p = tid - k * PPK; p < n; p += PPK) {
            const int dy = p / block, dx = p - dy * block;
            int row = bj * shift + dy, col = bi * shift + dx;  // beyond the image: edge replication
            row = row < H ? row : H - 1;
            col = col < W ? col : W - 1;
            const size_t o = (size_t)row * W + col;
            const unsigned g = q2n_quant(gk[o], scale);
            acc[0] += g;
            acc[1] += g * g;  // 65535^2 < 2^32
#pragma unroll
            for (int l = 0; l < CP; ++l) {
                if (l < C) {
                    const unsigned f = q2n_quant(pb[l * plane + o], scale);
                    acc[4 + l] += g * f;
                    if (l == k) {
                        acc[2] += f;
                        acc[3] += f * f;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < NA; ++a) {
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1) acc[a] += __shfl_xor(acc[a], m);  // PPK >= 32: a 32-lane half holds one band
    }
    if ((tid & 31) == 0) {
#pragma unroll
        for (int a = 0; a < NA; ++a) red[(tid >> 5) * NA + a] = acc[a];
    }
    __syncthreads();
    if (tid != 0) return;

    constexpr Q2nTable<CP> tab = q2n_make_table<CP>();
    constexpr int HPK = PPK / 32;  // halves per band
    const i64 ni = n;
    const double nd = (double)n;
    i64 Sg[CP], Sf[CP];
    double rt[CP], ru[CP];
    double var_sum = 0.0, m2sq = 0.0;  // sum_k (vg_k / rt_k^2 + vf_k / ru_k^2),  |m2|^2
#pragma unroll
    for (int kk = 0; kk < CP; ++kk) {
        u64 s[4] = {0, 0, 0, 0};
        for (int h = 0; h < HPK; ++h)
            for (int a = 0; a < 4; ++a) s[a] += red[(kk * HPK + h) * NA + a];
        Sg[kk] = (i64)s[0];
        Sf[kk] = (i64)s[2];
        const i64 vg = ni * (i64)s[1] - Sg[kk] * Sg[kk], vf = ni * (i64)s[3] - Sf[kk] * Sf[kk];
        rt[kk] = vg == 0 ? nd * 1e-8 : sqrt((double)vg);
        ru[kk] = Sg[kk] == 0 ? nd : rt[kk];
        const double d = (double)(Sf[kk] - Sg[kk]) / ru[kk];
        var_sum += (double)vg / (rt[kk] * rt[kk]) + (double)vf / (ru[kk] * ru[kk]);
        m2sq += (d + 1.0) * (d + 1.0);
    }
    const double m1sq = (double)CP, unb = nd / (nd - 1.0);
    const double T3 = unb * var_sum;
    const double bias = 2.0 * (sqrt(m1sq) * sqrt(m2sq)) / (m1sq + m2sq);
    double Q = bias;  // T3 == 0: q = (0, ..., 0, bias)
    if (T3 != 0.0) {
        double q[CP];
#pragma unroll
        for (int r = 0; r < CP; ++r) q[r] = 0.0;
#pragma unroll
        for (int kk = 0; kk < CP; ++kk) {
#pragma unroll
            for (int l = 0; l < CP; ++l) {
                u64 x = 0;
                for (int h = 0; h < HPK; ++h) x += red[(kk * HPK + h) * NA + 4 + l];
                const i64 c = ni * (i64)x - Sg[kk] * Sf[l];
                const double v = (double)c / (rt[kk] * ru[l]);
                if (tab.sgn[kk][l] * (l == 0 ? 1 : -1) > 0) q[tab.idx[kk][l]] += v;
                else q[tab.idx[kk][l]] -= v;
            }
        }
        const double f = unb * bias * 2.0 / T3;
        double ss = 0.0;
#pragma unroll
        for (int r = 0; r < CP; ++r) ss += (q[r] * f) * (q[r] * f);
        Q = sqrt(ss);
    }
    map[blockIdx.x] = Q;
}

// Q2n of an image = the mean of its nblk blocks: strided partials, xor butterfly inside the wave, the four waves in a fixed order
__global__ __launch_bounds__(256) void q2n_mean_kernel(const double* map, int nblk, double* q_out) {
    DDIF_DYN_SMEM(smem_);
    double* red = reinterpret_cast<double*>(smem_);
    const double* m = map + (size_t)blockIdx.x * nblk;
    double s = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) s += m[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) q_out[blockIdx.x] = ((red[0] + red[1]) + (red[2] + red[3])) / (double)nblk;
}

}  // namespace ddif
