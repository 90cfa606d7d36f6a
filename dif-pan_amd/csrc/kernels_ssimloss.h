// HybridL1SSIM (utils/loss_utils.py:73-83, 98-147; _ssim :30-59): loss = 0.0 + L1(img1, img2) * w_l1 + (1 - mean(ssim_map(img1, img2))) * w_ssim and its
// gradient with respect to img2, as three launches.
//
//   ssim_stats_kernel  a workgroup owns a 16 x 16 pixel tile of one sample for 4 channels.  It stages both tensors once with a 5-pixel halo (zeros outside the
//                      image: F.conv2d's padding = 5 -- no per-tap test in the filter loops), runs the separable 11-tap Gaussian over x, y, x.x, x.y, y.y
//                      (rows into LDS, then columns), forms per pixel the map value S and
//                          G12 = dS / dE[xy] = 2 A1 / (B1 B2)         G22 = dS / dE[yy] = -S / B2
//                          Gm  = dS / dmu2 (total) = 2 (mu1 (A2 - A1) + mu2 S (B1 - B2)) / (B1 B2)
//                      (A1 = 2 mu1 mu2 + C1, A2 = 2 s12 + C2, B1 = mu1^2 + mu2^2 + C1, B2 = s11 + s22 + C2), writes the three maps and leaves ONE pair of fp64
//                      partials (sum |y - x|, sum S) per workgroup.
//   ssim_final_kernel  one thread adds the partials in workgroup order, composes the loss in the reference's fp32 order and applies the p2 factor (as
//                      loss_final_w_kernel, kernels_train.h): out[0] = loss, out[1] = d out[0] / d loss.
//   ssim_grad_kernel   the same tiling over the three maps (the window is symmetric, so the adjoint of the zero-padded filter is the zero-padded filter):
//                          d loss / d y(q) = w_l1 sign(y - x)(q) / n - (w_ssim / n) [ (W*Gm)(q) + 2 y(q) (W*G22)(q) + x(q) (W*G12)(q) ]
//
// No atomics; every sum has a fixed order, so results are bit-identical from run to run.  Tensors are addressed by element strides: NHWC (the plan's net_out
// and target) and NCHW (the Python boundary) run the same code; the template parameter only picks which index runs fastest over the lanes, for coalescing.
// LDS per workgroup: 55.3 KiB (statistics), 52.5 KiB (gradient) -- two workgroups per CU.
#pragma once
#include "ddif_dev.h"

namespace ddif {

enum {
    SSIM_T = 16,                  // tile edge
    SSIM_R = 5,                   // window radius
    SSIM_K = 2 * SSIM_R + 1,      // taps
    SSIM_P = SSIM_T + 2 * SSIM_R, // staged edge
    SSIM_CG = 4,                  // channels per workgroup
    SSIM_SPLANE = 688,            // floats per staged plane (26 x 26 = 676, padded to 16 mod 32: the planes of two channels sit on disjoint LDS banks)
    SSIM_RPLANE = 432,            // floats per row-filtered plane (26 x 16 = 416, padded likewise)
    SSIM_FCH = 1024,              // partial pairs the final kernel holds in LDS at a time
};
static_assert(SSIM_SPLANE >= SSIM_P * SSIM_P && SSIM_RPLANE >= SSIM_P * SSIM_T, "plane sizes");
static_assert(2 * SSIM_CG * SSIM_SPLANE * sizeof(float) >= 2 * 256 * sizeof(double), "the statistics kernel reduces its partials in the staging area");

struct SsimArgs {
    const float* x;  // img1 (the plan: the target)
    const float* y;  // img2 (the plan: the network output)
    int B, C, H, W;
    long long sb, sc, sh, sw;  // element strides of batch, channel, row, column -- the same for x, y, the maps and dy
    long long n;               // B C H W
    int tiles_x;
    float w[SSIM_K];           // the 1-D window
    float* maps;               // [3][n] Gm | G22 | G12 in the tensors' own layout (statistics: nullable = value only)
    double* part;              // [workgroups][2]
    float w_l1, w_ssim, upstream;
    const float* scale;        // the two floats ssim_final_kernel wrote
    float* dy;
};

inline size_t ssim_stats_smem() { return (size_t)(2 * SSIM_CG * SSIM_SPLANE + 5 * SSIM_CG * SSIM_RPLANE) * sizeof(float); }
inline size_t ssim_grad_smem() { return (size_t)(3 * SSIM_CG * SSIM_SPLANE + 3 * SSIM_CG * SSIM_RPLANE) * sizeof(float); }

// item i of a [SSIM_CG][edge][edge] block -> (channel, row, column); NHWC: the channel runs fastest over the lanes, else the column
template <bool NHWC>
__device__ __forceinline__ void ssim_item(int i, int edge, int& c, int& r, int& col) {
    if (NHWC) {
        c = i % SSIM_CG;
        col = (i / SSIM_CG) % edge;
        r = i / (SSIM_CG * edge);
    } else {
        col = i % edge;
        r = (i / edge) % edge;
        c = i / (edge * edge);
    }
}

// the map and its three derivatives at one pixel, in the reference's operand order (:34-54)
__device__ __forceinline__ void ssim_point(float mu1, float mu2, float e11, float e12, float e22, float& S, float& gm, float& g22, float& g12) {
#pragma clang fp contract(off)
    const float C1 = (float)(0.01 * 0.01), C2 = (float)(0.03 * 0.03);
    const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
    const float s11 = e11 - mu1_sq, s22 = e22 - mu2_sq, s12 = e12 - mu1_mu2;
    const float A1 = 2.0f * mu1_mu2 + C1, A2 = 2.0f * s12 + C2;
    const float B1 = mu1_sq + mu2_sq + C1, B2 = s11 + s22 + C2;
    S = (A1 * A2) / (B1 * B2);
    const float inv = 1.0f / (B1 * B2);
    g12 = (2.0f * A1) * inv;
    g22 = -S / B2;
    gm = (2.0f * inv) * (mu1 * (A2 - A1) + (mu2 * S) * (B1 - B2));
}

template <bool NHWC>
__global__ __launch_bounds__(256) void ssim_stats_kernel(SsimArgs a) {
    DDIF_DYN_SMEM(smem_);
    float* st = reinterpret_cast<float*>(smem_);  // [x | y][SSIM_CG][SSIM_SPLANE]
    float* rf = st + 2 * SSIM_CG * SSIM_SPLANE;   // [x, y, xx, xy, yy][SSIM_CG][SSIM_RPLANE]: 26 rows x 16 columns
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x, c0 = blockIdx.y * SSIM_CG;
    const int h0 = ty * SSIM_T - SSIM_R, w0 = tx * SSIM_T - SSIM_R;
    const long long base = (long long)blockIdx.z * a.sb;
    for (int i = tid; i < SSIM_CG * SSIM_P * SSIM_P; i += 256) {
        int c, r, col;
        ssim_item<NHWC>(i, SSIM_P, c, r, col);
        const int h = h0 + r, w = w0 + col;
        float xv = 0.f, yv = 0.f;
        if (h >= 0 && h < a.H && w >= 0 && w < a.W && c0 + c < a.C) {
            const long long o = base + (c0 + c) * a.sc + h * a.sh + w * a.sw;
            xv = a.x[o];
            yv = a.y[o];
        }
        st[c * SSIM_SPLANE + r * SSIM_P + col] = xv;
        st[(SSIM_CG + c) * SSIM_SPLANE + r * SSIM_P + col] = yv;
    }
    __syncthreads();
    for (int i = tid; i < SSIM_CG * SSIM_P * SSIM_T; i += 256) {  // rows: lanes over (column, channel): conflict-free reads
        const int col = i % SSIM_T, c = (i / SSIM_T) % SSIM_CG, r = i / (SSIM_T * SSIM_CG);
        const float* px = st + c * SSIM_SPLANE + r * SSIM_P + col;
        const float* py = px + SSIM_CG * SSIM_SPLANE;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
#pragma unroll
        for (int k = 0; k < SSIM_K; ++k) {
            const float wv = a.w[k], xv = px[k], yv = py[k];
            s0 = fmaf(wv, xv, s0);
            s1 = fmaf(wv, yv, s1);
            s2 = fmaf(wv, xv * xv, s2);
            s3 = fmaf(wv, xv * yv, s3);
            s4 = fmaf(wv, yv * yv, s4);
        }
        float* q = rf + c * SSIM_RPLANE + r * SSIM_T + col;
        q[0 * SSIM_CG * SSIM_RPLANE] = s0;
        q[1 * SSIM_CG * SSIM_RPLANE] = s1;
        q[2 * SSIM_CG * SSIM_RPLANE] = s2;
        q[3 * SSIM_CG * SSIM_RPLANE] = s3;
        q[4 * SSIM_CG * SSIM_RPLANE] = s4;
    }
    __syncthreads();
    double acc_l1 = 0.0, acc_s = 0.0;
    for (int i = tid; i < SSIM_CG * SSIM_T * SSIM_T; i += 256) {  // columns, the map, the partial sums
        int c, r, col;
        ssim_item<NHWC>(i, SSIM_T, c, r, col);
        const int h = h0 + SSIM_R + r, w = w0 + SSIM_R + col;
        if (h >= a.H || w >= a.W || c0 + c >= a.C) continue;
        float e[5];
#pragma unroll
        for (int p = 0; p < 5; ++p) {
            const float* q = rf + (p * SSIM_CG + c) * SSIM_RPLANE + r * SSIM_T + col;
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < SSIM_K; ++k) s = fmaf(a.w[k], q[k * SSIM_T], s);
            e[p] = s;
        }
        float S, gm, g22, g12;
        ssim_point(e[0], e[1], e[2], e[3], e[4], S, gm, g22, g12);
        const float xv = st[c * SSIM_SPLANE + (r + SSIM_R) * SSIM_P + col + SSIM_R];
        const float yv = st[(SSIM_CG + c) * SSIM_SPLANE + (r + SSIM_R) * SSIM_P + col + SSIM_R];
        acc_l1 += (double)fabsf(yv - xv);
        acc_s += (double)S;
        if (a.maps) {
            const long long o = base + (c0 + c) * a.sc + h * a.sh + w * a.sw;
            a.maps[o] = gm;
            a.maps[a.n + o] = g22;
            a.maps[2 * a.n + o] = g12;
        }
    }
    __syncthreads();  // (the staging area is free: every read of it is above)
    double* red = reinterpret_cast<double*>(smem_);  // [2][256]
    red[tid] = acc_l1;
    red[256 + tid] = acc_s;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) {
            red[tid] += red[tid + s];
            red[256 + tid] += red[256 + tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const size_t wg = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        a.part[2 * wg] = red[0];
        a.part[2 * wg + 1] = red[256];
    }
}

// loss = 0.0 + l1 * w_l1 + (1 - mean S) * w_ssim in fp32, this order (LossWarpper.forward :108-115, SSIMLoss.forward :145); then the p2 weighting (:762-764) as
// loss_final_w_kernel.  All threads move the partials into LDS, ONE thread adds them in workgroup order.
__global__ __launch_bounds__(256) void ssim_final_kernel(const double* part, int nwg, long long n, float w_l1, float w_ssim, const float* w, int B, float* out) {
#pragma clang fp contract(off)
    DDIF_DYN_SMEM(smem_);
    double* buf = reinterpret_cast<double*>(smem_);  // [SSIM_FCH][2]
    const int tid = threadIdx.x;
    double s1 = 0.0, s2 = 0.0;
    for (int b0 = 0; b0 < nwg; b0 += SSIM_FCH) {
        const int m = nwg - b0 < SSIM_FCH ? nwg - b0 : SSIM_FCH;
        for (int i = tid; i < 2 * m; i += 256) buf[i] = part[2 * (size_t)b0 + i];
        __syncthreads();
        if (tid == 0)
            for (int k = 0; k < m; ++k) {
                s1 += buf[2 * k];
                s2 += buf[2 * k + 1];
            }
        __syncthreads();
    }
    if (tid == 0) {
        const float l1 = (float)(s1 / (double)n), ms = (float)(s2 / (double)n);
        float loss = 0.0f + l1 * w_l1;
        loss = loss + (1.0f - ms) * w_ssim;
        if (!w) {
            out[0] = loss;
            out[1] = 1.f;
        } else {
            float acc = 0.f, wsum = 0.f;
            for (int b = 0; b < B; ++b) {
                acc += loss * w[b];
                wsum += w[b];
            }
            out[0] = acc / (float)B;
            out[1] = wsum / (float)B;
        }
    }
}

__device__ __forceinline__ float ssim_dy(float xv, float yv, float fm, float f22, float f12, float gl1, float gs, float up) {
#pragma clang fp contract(off)
    const float df = yv - xv;
    const float l1 = df > 0.f ? gl1 : (df < 0.f ? -gl1 : 0.f);  // torch: sign(0) = 0
    return (l1 - gs * (fm + (2.0f * yv) * f22 + xv * f12)) * up;
}

template <bool NHWC>
__global__ __launch_bounds__(256) void ssim_grad_kernel(SsimArgs a) {
    DDIF_DYN_SMEM(smem_);
    float* st = reinterpret_cast<float*>(smem_);  // [Gm | G22 | G12][SSIM_CG][SSIM_SPLANE]
    float* rf = st + 3 * SSIM_CG * SSIM_SPLANE;   // [3][SSIM_CG][SSIM_RPLANE]
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x, c0 = blockIdx.y * SSIM_CG;
    const int h0 = ty * SSIM_T - SSIM_R, w0 = tx * SSIM_T - SSIM_R;
    const long long base = (long long)blockIdx.z * a.sb;
    for (int i = tid; i < SSIM_CG * SSIM_P * SSIM_P; i += 256) {
        int c, r, col;
        ssim_item<NHWC>(i, SSIM_P, c, r, col);
        const int h = h0 + r, w = w0 + col;
        float v0 = 0.f, v1 = 0.f, v2 = 0.f;
        if (h >= 0 && h < a.H && w >= 0 && w < a.W && c0 + c < a.C) {
            const long long o = base + (c0 + c) * a.sc + h * a.sh + w * a.sw;
            v0 = a.maps[o];
            v1 = a.maps[a.n + o];
            v2 = a.maps[2 * a.n + o];
        }
        float* q = st + c * SSIM_SPLANE + r * SSIM_P + col;
        q[0] = v0;
        q[SSIM_CG * SSIM_SPLANE] = v1;
        q[2 * SSIM_CG * SSIM_SPLANE] = v2;
    }
    __syncthreads();
    for (int i = tid; i < 3 * SSIM_CG * SSIM_P * SSIM_T; i += 256) {  // rows of the three maps (plane = map * SSIM_CG + channel)
        const int col = i % SSIM_T, pl = (i / SSIM_T) % (3 * SSIM_CG), r = i / (SSIM_T * 3 * SSIM_CG);
        const float* p = st + pl * SSIM_SPLANE + r * SSIM_P + col;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < SSIM_K; ++k) s = fmaf(a.w[k], p[k], s);
        rf[pl * SSIM_RPLANE + r * SSIM_T + col] = s;
    }
    __syncthreads();
    const float up = a.upstream * a.scale[1];
    const float gl1 = a.w_l1 / (float)a.n, gs = a.w_ssim / (float)a.n;
    for (int i = tid; i < SSIM_CG * SSIM_T * SSIM_T; i += 256) {
        int c, r, col;
        ssim_item<NHWC>(i, SSIM_T, c, r, col);
        const int h = h0 + SSIM_R + r, w = w0 + SSIM_R + col;
        if (h >= a.H || w >= a.W || c0 + c >= a.C) continue;
        float f[3];
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const float* q = rf + (p * SSIM_CG + c) * SSIM_RPLANE + r * SSIM_T + col;
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < SSIM_K; ++k) s = fmaf(a.w[k], q[k * SSIM_T], s);
            f[p] = s;
        }
        const long long o = base + (c0 + c) * a.sc + h * a.sh + w * a.sw;
        a.dy[o] = ssim_dy(a.x[o], a.y[o], f[0], f[1], f[2], gl1, gs, up);
    }
}

}  // namespace ddif
