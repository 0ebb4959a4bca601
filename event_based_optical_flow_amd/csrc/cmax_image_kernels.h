// Image-space kernels shared by the leaf operators and the fused objective (header-only
// templates): 3-tap reflect-101 Gaussian blur + transpose, Sobel/8 with zero padding.
#pragma once
#include "cmax_common.h"

namespace cmax {

__device__ __forceinline__ int refl101(int i, int n) {
    if (n == 1) return 0;
    if (i < 0) return -i;
    if (i >= n) return 2 * n - 2 - i;
    return i;
}

// torchvision gaussian_blur(kernel_size=3, sigma) taps (src/event_image_converter.py:158)
static inline void blur_taps(double sigma, double &k0, double &k1) {
    double e = exp(-0.5 / (sigma * sigma));
    double s = 1.0 + 2.0 * e;
    k0 = 1.0 / s;
    k1 = e / s;
}

// forward: out[i,j] = sum_{a,b} k[a] k[b] in[refl(i+a), refl(j+b)]
// bs: element stride between the images of a batch (blockIdx.y), 0 for a single image
template <typename T>
__global__ void __launch_bounds__(256) k_blur3(const T *__restrict__ in, int H, int W, T k0, T k1, T *__restrict__ out, int64_t bs = 0) {
    in += blockIdx.y * bs;
    out += blockIdx.y * bs;
    int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (int64_t)H * W) return;
    int i = (int)(p / W), j = (int)(p % W);
    int im = refl101(i - 1, H), ip = refl101(i + 1, H), jm = refl101(j - 1, W), jp = refl101(j + 1, W);
    auto row = [&](int r) { return k1 * in[(int64_t)r * W + jm] + k0 * in[(int64_t)r * W + j] + k1 * in[(int64_t)r * W + jp]; };
    out[p] = k1 * row(im) + k0 * row(i) + k1 * row(ip);
}

// 1-D transposed operator: (K^T g)[p] = k0 g[p] + k1 (g[p-1] + g[p+1]) (in range) + the reflected
// taps folded back: index 1 also receives k1 g[0], index n-2 also receives k1 g[n-1].
template <typename T, typename F>
__device__ __forceinline__ T blur_adj_1d(int p, int n, T k0, T k1, F g) {
    if (n == 1) return (k0 + (T)2 * k1) * g(0);
    T s = k0 * g(p);
    if (p - 1 >= 0) s += k1 * g(p - 1);
    if (p + 1 < n) s += k1 * g(p + 1);
    if (p == 1) s += k1 * g(0);
    if (p == n - 2) s += k1 * g(n - 1);
    return s;
}

template <typename T>
__global__ void __launch_bounds__(256) k_blur3_adj(const T *__restrict__ g, int H, int W, T k0, T k1, T *__restrict__ out, int64_t bs = 0) {
    g += blockIdx.y * bs;
    out += blockIdx.y * bs;
    int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (int64_t)H * W) return;
    int i = (int)(p / W), j = (int)(p % W);
    out[p] = blur_adj_1d<T>(i, H, k0, k1, [&](int r) {
        return blur_adj_1d<T>(j, W, k0, k1, [&](int c) { return g[(int64_t)r * W + c]; });
    });
}

// Sobel / 8 with zero padding (SobelTorch, src/utils/stat_utils.py:50-62,80-83); fp64 arithmetic
// like the solvers' precision="64" (src/solver/base.py:180, gradient_magnitude.py:65-66).
template <typename T>
__device__ __forceinline__ void sobel8(const T *__restrict__ img, int H, int W, int i, int j, double &gx, double &gy) {
    auto at = [&](int r, int c) -> double {
        return (r < 0 || r >= H || c < 0 || c >= W) ? 0.0 : (double)img[(int64_t)r * W + c];
    };
    double a00 = at(i - 1, j - 1), a01 = at(i - 1, j), a02 = at(i - 1, j + 1);
    double a10 = at(i, j - 1), a12 = at(i, j + 1);
    double a20 = at(i + 1, j - 1), a21 = at(i + 1, j), a22 = at(i + 1, j + 1);
    gx = ((a20 + 2.0 * a21 + a22) - (a00 + 2.0 * a01 + a02)) / 8.0;  // row derivative
    gy = ((a02 + 2.0 * a12 + a22) - (a00 + 2.0 * a10 + a20)) / 8.0;  // column derivative
}

// d mean(gx^2+gy^2) / d img[p] * n / 2 * 8 : sum over the output pixels q in Omega that read p.
template <typename T>
__device__ __forceinline__ double sobel8_adj(const T *__restrict__ img, int H, int W, int i0, int i, int j) {
    const double SX[3][3] = {{-1, -2, -1}, {0, 0, 0}, {1, 2, 1}};
    const double SY[3][3] = {{-1, 0, 1}, {-2, 0, 2}, {-1, 0, 1}};
    double s = 0.0;
#pragma unroll
    for (int a = -1; a <= 1; ++a)
#pragma unroll
        for (int b = -1; b <= 1; ++b) {
            int qi = i - a, qj = j - b;  // output pixel q read p with tap (a, b)
            if (qi < i0 || qi >= H - i0 || qj < i0 || qj >= W - i0) continue;
            double gx, gy;
            sobel8<T>(img, H, W, qi, qj, gx, gy);
            s += gx * SX[a + 1][b + 1] + gy * SY[a + 1][b + 1];
        }
    return s;
}

// fp32 variants for the fused path (the IWE is fp32; sums of squares are accumulated in fp64 by the caller)
__device__ __forceinline__ void sobel8_f32(const float *__restrict__ img, int H, int W, int i, int j, float &gx, float &gy) {
    auto at = [&](int r, int c) -> float {
        return (r < 0 || r >= H || c < 0 || c >= W) ? 0.f : img[(int64_t)r * W + c];
    };
    const float a00 = at(i - 1, j - 1), a01 = at(i - 1, j), a02 = at(i - 1, j + 1);
    const float a10 = at(i, j - 1), a12 = at(i, j + 1);
    const float a20 = at(i + 1, j - 1), a21 = at(i + 1, j), a22 = at(i + 1, j + 1);
    gx = ((a20 + 2.f * a21 + a22) - (a00 + 2.f * a01 + a02)) * 0.125f;
    gy = ((a02 + 2.f * a12 + a22) - (a00 + 2.f * a10 + a20)) * 0.125f;
}

// sum_{q in Omega reading p} gx(q) SX + gy(q) SY from one 5x5 neighbourhood held in registers
// (25 loads per pixel instead of 9 x 8); gx, gy include the /8.
// gx0, gy0 (optional): the Sobel/8 response AT (i, j) from the same registers
__device__ __forceinline__ float sobel8_adj_f32(const float *__restrict__ img, int H, int W, int i0, int i, int j,
                                                float *gx0 = nullptr, float *gy0 = nullptr) {
    float v[5][5];
#pragma unroll
    for (int a = 0; a < 5; ++a)
#pragma unroll
        for (int b = 0; b < 5; ++b) {
            const int r = i + a - 2, c = j + b - 2;
            v[a][b] = (r < 0 || r >= H || c < 0 || c >= W) ? 0.f : img[(int64_t)r * W + c];
        }
    if (gx0) {
        *gx0 = ((v[3][1] + 2.f * v[3][2] + v[3][3]) - (v[1][1] + 2.f * v[1][2] + v[1][3])) * 0.125f;
        *gy0 = ((v[1][3] + 2.f * v[2][3] + v[3][3]) - (v[1][1] + 2.f * v[2][1] + v[3][1])) * 0.125f;
    }
    float s = 0.f;
#pragma unroll
    for (int a = -1; a <= 1; ++a)
#pragma unroll
        for (int b = -1; b <= 1; ++b) {
            const int qi = i - a, qj = j - b;  // output pixel q read p with tap (a, b)
            if (qi < i0 || qi >= H - i0 || qj < i0 || qj >= W - i0) continue;
            const int ci = 2 - a, cj = 2 - b;  // q inside the 5x5 block
            const float gx = ((v[ci + 1][cj - 1] + 2.f * v[ci + 1][cj] + v[ci + 1][cj + 1]) -
                              (v[ci - 1][cj - 1] + 2.f * v[ci - 1][cj] + v[ci - 1][cj + 1])) * 0.125f;
            const float gy = ((v[ci - 1][cj + 1] + 2.f * v[ci][cj + 1] + v[ci + 1][cj + 1]) -
                              (v[ci - 1][cj - 1] + 2.f * v[ci][cj - 1] + v[ci + 1][cj - 1])) * 0.125f;
            const float sx = (float)a * (b == 0 ? 2.f : 1.f);  // SX[a+1][b+1] = a * (2 - |b|)
            const float sy = (float)b * (a == 0 ? 2.f : 1.f);  // SY[a+1][b+1] = b * (2 - |a|)
            s += gx * sx + gy * sy;
        }
    return s;
}

// ---------------------------------------------------------------------------------------------
// Focus losses (CMAX_COST_MEAN_SQUARE / _LAPLACIAN / _HESSIAN): v = (1/n) sum_{q in Omega} sum_s c_s r_s(q)^2, every response
// r_s = S_s * I a 3 x 3 stencil on the image read as zero outside it.  One trait per cost:
//   kResp         number of responses
//   resp(n, r)    the responses at a pixel from its neighbourhood n[a + 1][b + 1] = I(r + a, c + b)
//   tap(s, a, b)  S_s[a][b]: what response s of pixel q reads of pixel q + (a, b) -- the transpose taps
//   weight(s)     c_s
// dv/dI[p] = (2/n) sum_{(a, b)} 1_Omega(p - (a, b)) sum_s c_s r_s(p - (a, b)) tap(s, a, b).  The kernels are written once over the
// trait; A is the arithmetic type (float on the fused path, double in the leaf operator).
// sum_s c_s |S_s|_1^2 (the deterministic K3's bound): 1, 64, 34.
// ---------------------------------------------------------------------------------------------
template <int COST>
struct FocusStencil;

template <>
struct FocusStencil<CMAX_COST_MEAN_SQUARE> {
    static constexpr int kResp = 1;
    template <typename A>
    __device__ __forceinline__ static void resp(const A (&n)[3][3], A (&r)[1]) { r[0] = n[1][1]; }
    __host__ __device__ static constexpr float tap(int, int a, int b) { return (a == 0 && b == 0) ? 1.f : 0.f; }
    __host__ __device__ static constexpr float weight(int) { return 1.f; }
};

template <>
struct FocusStencil<CMAX_COST_LAPLACIAN> {
    static constexpr int kResp = 1;
    template <typename A>
    __device__ __forceinline__ static void resp(const A (&n)[3][3], A (&r)[1]) { r[0] = ((n[0][1] + n[2][1]) + (n[1][0] + n[1][2])) - (A)4 * n[1][1]; }
    __host__ __device__ static constexpr float tap(int, int a, int b) { return (a == 0 && b == 0) ? -4.f : ((a == 0 || b == 0) ? 1.f : 0.f); }
    __host__ __device__ static constexpr float weight(int) { return 1.f; }
};

template <>
struct FocusStencil<CMAX_COST_HESSIAN> {
    static constexpr int kResp = 3;  // h_rr, h_cc, h_rc
    template <typename A>
    __device__ __forceinline__ static void resp(const A (&n)[3][3], A (&r)[3]) {
        r[0] = (n[0][1] + n[2][1]) - (A)2 * n[1][1];
        r[1] = (n[1][0] + n[1][2]) - (A)2 * n[1][1];
        r[2] = (A)0.25 * ((n[2][2] - n[2][0]) - (n[0][2] - n[0][0]));
    }
    __host__ __device__ static constexpr float tap(int s, int a, int b) {
        return s == 0 ? (b != 0 ? 0.f : (a == 0 ? -2.f : 1.f)) : (s == 1 ? (a != 0 ? 0.f : (b == 0 ? -2.f : 1.f)) : 0.25f * (float)(a * b));
    }
    __host__ __device__ static constexpr float weight(int s) { return s == 2 ? 2.f : 1.f; }
};

// sum_s c_s r_s(n) r_s(m): the energy of a pixel with m = n, the tangent statistic with m = the tangent image's neighbourhood
template <int COST, typename A>
__device__ __forceinline__ A focus_dot(const A (&n)[3][3], const A (&m)[3][3]) {
    using S = FocusStencil<COST>;
    A rn[S::kResp], rm[S::kResp], e = (A)0;
    S::resp(n, rn);
    S::resp(m, rm);
#pragma unroll
    for (int s = 0; s < S::kResp; ++s) e += (A)S::weight(s) * rn[s] * rm[s];
    return e;
}
template <int COST, typename A>
__device__ __forceinline__ A focus_energy(const A (&n)[3][3]) { return focus_dot<COST, A>(n, n); }

// what output pixel q = p - (a, b) hands back to p: sum_s c_s r_s(q) tap(s, a, b) (the zero taps fold away)
template <int COST, typename A>
__device__ __forceinline__ A focus_tap_sum(const A (&r)[FocusStencil<COST>::kResp], int a, int b) {
    using S = FocusStencil<COST>;
    A t = (A)0;
#pragma unroll
    for (int s = 0; s < S::kResp; ++s)
        if (S::tap(s, a, b) != 0.f) t += (A)(S::weight(s) * S::tap(s, a, b)) * r[s];
    return t;
}

// the (2R + 1)^2 neighbourhood of (i, j), zero outside the image
template <int R, typename A, typename T>
__device__ __forceinline__ void focus_load(const T *__restrict__ img, int H, int W, int i, int j, A (&v)[2 * R + 1][2 * R + 1]) {
#pragma unroll
    for (int a = 0; a < 2 * R + 1; ++a)
#pragma unroll
        for (int b = 0; b < 2 * R + 1; ++b) {
            const int r = i + a - R, c = j + b - R;
            v[a][b] = (r < 0 || r >= H || c < 0 || c >= W) ? (A)0 : (A)img[(int64_t)r * W + c];
        }
}

// dv/dI[p] * n / 2 at p = (i, j) from its 5 x 5 neighbourhood v (v[2][2] = I(p)): the sum over the output pixels q in Omega that read p
template <int COST, typename A>
__device__ __forceinline__ A focus_adj(const A (&v)[5][5], int H, int W, int i0, int i, int j) {
    using S = FocusStencil<COST>;
    A s = (A)0;
#pragma unroll
    for (int a = -1; a <= 1; ++a)
#pragma unroll
        for (int b = -1; b <= 1; ++b) {
            bool any = false;
#pragma unroll
            for (int t = 0; t < S::kResp; ++t) any = any || S::tap(t, a, b) != 0.f;
            if (!any) continue;
            const int qi = i - a, qj = j - b;
            if (qi < i0 || qi >= H - i0 || qj < i0 || qj >= W - i0) continue;
            A n[3][3], r[S::kResp];
#pragma unroll
            for (int x = 0; x < 3; ++x)
#pragma unroll
                for (int y = 0; y < 3; ++y) n[x][y] = v[1 - a + x][1 - b + y];
            S::resp(n, r);
            s += focus_tap_sum<COST, A>(r, a, b);
        }
    return s;
}

}  // namespace cmax
