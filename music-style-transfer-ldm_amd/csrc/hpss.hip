// Harmonic / percussive separation: the running median along one axis of a [B, F, T] spectrogram,
// librosa's soft masks of the two medians, and the masked component's energy share on the mel grid.
//
// Median: out[i] = the middle order statistic of the `win` samples centred on i, the axis continued by scipy's
// "reflect" (d c b a | a b c d | d c b a: period 2n, the edge sample repeated).  A block stages its tile plus a halo of
// win / 2 on both sides of the filtered axis in LDS, the reflection resolved while the halo is filled (every slot's
// source index is folded into [0, n) once, so the fill never reads outside the row and the selection never tests a
// bound).  Each lane then copies its window from LDS to registers and selects by rank counting: sample i is the
// median when exactly win / 2 samples stand before it in the order (value, position), i.e.
//   rank(i) = #{j < i : w[j] <= w[i]} + #{j > i : w[j] < w[i]} == win / 2.
// The position tie-break makes the ranks a permutation of 0 .. win - 1, so exactly one sample matches however many
// are equal; the result is one of the inputs, no arithmetic touches it.  The window array has the length of the
// window's class (3, 7, 15, 31, 63), samples beyond win are +inf and never stand before a sample of the window.
// The selection is branch-free per lane (compare + add with carry per pair, fully unrolled: about 2 win W VALU
// instructions per output) and data-independent in time.  NaN inputs: every compare with a NaN is false, the
// ranks are no permutation any more and the output is unspecified (some sample of the window).
//
// Geometry, stated once (kTileT, kTileF; ldm_amd.ops imports the same numbers through ldm_median_tile):
//   time  (axis 1): block (64, 4) = 4 rows x kTileT frames, LDS [4][kTileT + 2 halo]; a lane owns frames tx + 64 k of
//                   its row; lanes of a wave read consecutive LDS words, global rows in 256-byte runs.
//   freq  (axis 0): block (64, 4) = kTileF bins x 64 frames, LDS [kTileF + 2 halo][64]: a slab read and written in
//                   256-byte runs along T; a lane owns frame tx and the bins ty + 4 k, its window is a column of the
//                   slab (stride 64 words: the lanes of a wave again read consecutive words).
#include "common.h"

#include <cfloat>
#include <cmath>

namespace ldm {
namespace {

constexpr int kTileT = 256;   // frames per block, time pass
constexpr int kTileF = 64;    // bins per block, frequency pass
constexpr int kMaxWin = 63;

// scipy's "reflect" continuation of an axis of n samples: p (any int) -> [0, n)
__device__ __forceinline__ int reflect_index(int p, int n) {
    const int period = 2 * n;
    int q = p % period;
    if (q < 0) q += period;
    return q < n ? q : period - 1 - q;
}

// The median of p[0], p[stride], .. p[(win - 1) stride] (LDS), win <= W odd.
template <int W>
__device__ __forceinline__ float median_select(const float* p, int stride, int win) {
    float w[W];
#pragma unroll
    for (int k = 0; k < W; ++k) w[k] = k < win ? p[k * stride] : INFINITY;
    const int half = win >> 1;
    float med = w[0];
#pragma unroll
    for (int i = 0; i < W; ++i) {
        if (i < win) {   // uniform over the launch
            int rank = 0;
#pragma unroll
            for (int j = 0; j < W; ++j) {
                if (j < i) rank += w[j] <= w[i] ? 1 : 0;
                if (j > i) rank += w[j] < w[i] ? 1 : 0;
            }
            med = rank == half ? w[i] : med;
        }
    }
    return med;
}

// block (64, 4), grid (ceil(T / kTileT), ceil(F / 4), B); dynamic LDS 4 (kTileT + win - 1) floats
template <int W>
__global__ __launch_bounds__(256) void median_time_kernel(const float* __restrict__ x, float* __restrict__ out, int F,
                                                          int T, int win) {
    extern __shared__ float tile[];
    const int halo = win >> 1, pitch = kTileT + 2 * halo;
    const int t0 = blockIdx.x * kTileT, f = blockIdx.y * 4 + threadIdx.y, b = blockIdx.z;
    const bool row = f < F;
    const int64_t base = ((int64_t)b * F + (row ? f : 0)) * T;
    float* mine = tile + threadIdx.y * pitch;
    if (row)
        for (int s = threadIdx.x; s < pitch; s += 64) mine[s] = x[base + reflect_index(t0 - halo + s, T)];
    __syncthreads();
    if (!row) return;
    for (int k = 0; k < kTileT / 64; ++k) {
        const int tl = threadIdx.x + 64 * k, t = t0 + tl;
        if (t < T) out[base + t] = median_select<W>(mine + tl, 1, win);
    }
}

// block (64, 4), grid (ceil(T / 64), ceil(F / kTileF), B); dynamic LDS (kTileF + win - 1) 64 floats
template <int W>
__global__ __launch_bounds__(256) void median_freq_kernel(const float* __restrict__ x, float* __restrict__ out, int F,
                                                          int T, int win) {
    extern __shared__ float tile[];
    const int halo = win >> 1, rows = kTileF + 2 * halo;
    const int t = blockIdx.x * 64 + threadIdx.x, f0 = blockIdx.y * kTileF, b = blockIdx.z;
    const bool col = t < T;
    const int64_t base = (int64_t)b * F * T + (col ? t : 0);
    if (col)
        for (int s = threadIdx.y; s < rows; s += 4)
            tile[s * 64 + threadIdx.x] = x[base + (int64_t)reflect_index(f0 - halo + s, F) * T];
    __syncthreads();
    if (!col) return;
    for (int k = 0; k < kTileF / 4; ++k) {
        const int fl = threadIdx.y + 4 * k, f = f0 + fl;
        if (f < F) out[base + (int64_t)f * T] = median_select<W>(tile + fl * 64 + threadIdx.x, 64, win);
    }
}

template <int W>
void launch_median(const float* x, float* out, int B, int F, int T, int axis, int win, hipStream_t stream) {
    if (axis == 1) {
        hipLaunchKernelGGL(median_time_kernel<W>, dim3((T + kTileT - 1) / kTileT, (F + 3) / 4, B), dim3(64, 4),
                           4 * (kTileT + win - 1) * sizeof(float), stream, x, out, F, T, win);
    } else {
        hipLaunchKernelGGL(median_freq_kernel<W>, dim3((T + 63) / 64, (F + kTileF - 1) / kTileF, B), dim3(64, 4),
                           (kTileF + win - 1) * 64 * sizeof(float), stream, x, out, F, T, win);
    }
}

// librosa's softmask, every step a correctly rounded fp32 operation (no contraction)
#pragma clang fp contract(off)
template <int P>   // 1, 2: multiplications only; 0: powf
__device__ __forceinline__ float soft(float X, float R, float power) {
    const float Z = fmaxf(X, R);
    if (Z < FLT_MIN) return 0.5f;
    float a = X / Z, r = R / Z;
    if constexpr (P == 2) {
        a = a * a;
        r = r * r;
    } else if constexpr (P == 0) {
        a = powf(a, power);
        r = powf(r, power);
    }
    return a / (a + r);
}

template <int P>
__global__ __launch_bounds__(256) void hpss_masks_kernel(const float* __restrict__ harm, const float* __restrict__ perc,
                                                         int64_t n, float power, float margin_h, float margin_p,
                                                         float* __restrict__ mask_h, float* __restrict__ mask_p) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float h = harm[i], p = perc[i];
    if (mask_h) mask_h[i] = soft<P>(h, margin_h * p, power);
    if (mask_p) mask_p[i] = soft<P>(p, margin_p * h, power);
}

// out[b, m, t] = (sum_k M[m, k] mask[b, k, t] P[b, k, t]) / (sum_k M[m, k] P[b, k, t]) over k in [lo_m, hi_m): the
// lanes and the grid of mel_project_kernel (audio.hip).  Both sums add the same product M P in the same order, the
// numerator's scaled by the mask, so with rounding monotone num <= den at every step when mask <= 1, and mask == 1
// gives the same bits in both.  block (64, 4), grid (ceil(T / 64), ceil(n_mels / 4), B)
__global__ __launch_bounds__(256) void mask_mel_share_kernel(const float* __restrict__ P, const float* __restrict__ mask,
                                                             const float* __restrict__ M,
                                                             const int32_t* __restrict__ lohi, float* __restrict__ out,
                                                             int F, int n_mels, int T) {
    const int t = blockIdx.x * 64 + threadIdx.x, m = blockIdx.y * 4 + threadIdx.y, b = blockIdx.z;
    if (m >= n_mels || t >= T) return;
    const int lo = max(lohi[2 * m], 0), hi = min(lohi[2 * m + 1], F);
    const float* p = P + (int64_t)b * F * T + t;
    const float* g = mask + (int64_t)b * F * T + t;
    const float* w = M + (int64_t)m * F;
    float num = 0.f, den = 0.f;
    for (int k = lo; k < hi; ++k) {
        const float wp = w[k] * p[(int64_t)k * T];
        den = den + wp;
        num = num + g[(int64_t)k * T] * wp;
    }
    const float share = den < FLT_MIN ? 0.5f : num / den;
    out[((int64_t)b * n_mels + m) * T + t] = fminf(fmaxf(share, 0.f), 1.f);
}

}  // namespace
}  // namespace ldm

using namespace ldm;

extern "C" int ldm_median_tile(int32_t axis) { return axis == 1 ? kTileT : axis == 0 ? kTileF : 0; }

extern "C" int ldm_median_filter(const float* x, int32_t B, int32_t F, int32_t T, int32_t axis, int32_t win, float* out,
                                 void* stream) {
    LDM_REQUIRE(x && out, "median_filter: null pointer");
    LDM_REQUIRE(axis == 0 || axis == 1, "median_filter: axis must be 0 (frequency) or 1 (time)");
    LDM_REQUIRE(win >= 1 && win <= kMaxWin && (win & 1), "median_filter: win must be odd and lie in 1..63");
    LDM_REQUIRE(B >= 1 && B <= 65535 && F >= 1 && F <= 4 * 65535 && T >= 1 && T < (1 << 30),
                "median_filter: bad shape (B 1..65535, F 1..262140, T below 2^30)");
    const uint64_t bytes = (uint64_t)B * F * T * sizeof(float), xa = (uint64_t)(uintptr_t)x, oa = (uint64_t)(uintptr_t)out;
    LDM_REQUIRE(oa + bytes <= xa || xa + bytes <= oa, "median_filter: out must not alias x");
    hipStream_t s = (hipStream_t)stream;
    if (win <= 3) launch_median<3>(x, out, B, F, T, axis, win, s);
    else if (win <= 7) launch_median<7>(x, out, B, F, T, axis, win, s);
    else if (win <= 15) launch_median<15>(x, out, B, F, T, axis, win, s);
    else if (win <= 31) launch_median<31>(x, out, B, F, T, axis, win, s);
    else launch_median<63>(x, out, B, F, T, axis, win, s);
    LDM_CHECK_LAUNCH("median_kernel");
    return 0;
}

extern "C" int ldm_hpss_masks(const float* harm, const float* perc, int64_t n, float power, float margin_h,
                              float margin_p, float* mask_h, float* mask_p, void* stream) {
    LDM_REQUIRE(harm && perc, "hpss_masks: null pointer");
    LDM_REQUIRE(n >= 1 && n <= ((int64_t)1 << 38), "hpss_masks: n out of range");
    LDM_REQUIRE(std::isfinite(power) && power > 0.f, "hpss_masks: power must be finite and positive");
    LDM_REQUIRE(margin_h >= 1.f && margin_p >= 1.f && std::isfinite(margin_h) && std::isfinite(margin_p),
                "hpss_masks: margins must be finite and at least 1");
    if (!mask_h && !mask_p) return 0;
    const dim3 grid((unsigned)((n + 255) / 256));
    hipStream_t s = (hipStream_t)stream;
    if (power == 1.f)
        hipLaunchKernelGGL(hpss_masks_kernel<1>, grid, dim3(256), 0, s, harm, perc, n, power, margin_h, margin_p, mask_h,
                           mask_p);
    else if (power == 2.f)
        hipLaunchKernelGGL(hpss_masks_kernel<2>, grid, dim3(256), 0, s, harm, perc, n, power, margin_h, margin_p, mask_h,
                           mask_p);
    else
        hipLaunchKernelGGL(hpss_masks_kernel<0>, grid, dim3(256), 0, s, harm, perc, n, power, margin_h, margin_p, mask_h,
                           mask_p);
    LDM_CHECK_LAUNCH("hpss_masks_kernel");
    return 0;
}

extern "C" int ldm_mask_mel_share(const float* P, const float* mask, const float* M, const int32_t* lohi, int32_t B,
                                  int32_t F, int32_t T, int32_t n_mels, float* out, void* stream) {
    LDM_REQUIRE(P && mask && M && lohi && out, "mask_mel_share: null pointer");
    LDM_REQUIRE(B >= 1 && B <= 65535 && F >= 1 && n_mels >= 1 && n_mels <= 4 * 65535 && T >= 1,
                "mask_mel_share: bad shape");
    hipLaunchKernelGGL(mask_mel_share_kernel, dim3((T + 63) / 64, (n_mels + 3) / 4, B), dim3(64, 4), 0,
                       (hipStream_t)stream, P, mask, M, lohi, out, F, n_mels, T);
    LDM_CHECK_LAUNCH("mask_mel_share_kernel");
    return 0;
}
