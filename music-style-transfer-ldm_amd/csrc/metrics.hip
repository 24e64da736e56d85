// Transfer report: the feature kernels behind the content-preservation and style-fit scores.
//   ldm_onset_strength  log-mel [B, n_mels, T] -> onset envelope [B, T] (mean positive difference at a lag)
//   ldm_chroma          power [B, F, T] -> 12 pitch classes per frame, each frame L2-normalised
//   ldm_mfcc_moments    log-mel -> { sum w, sum w c, sum w c c^T } of the MFCC frames c = D db, float64; the frames
//                       themselves never leave the chip
//   ldm_pair_stats      the seven weighted sums of two signals that Pearson, cosine and RMS difference come from
// Spectra are [B, rows, T] with T contiguous and lanes run along T, as everywhere in audio.hip: a wave reads 256-byte
// runs of one row, and whatever indexes a row (mel bin, FFT bin, coefficient) is uniform over the wave, so tables
// indexed by it (cls, wt, D) come through scalar loads.
//
// The two fp32 kernels do every step as one rounded fp32 operation in a stated order (contraction off).  The two
// reductions are float64 throughout with a fixed partition that depends on the item's own length only (tiles of
// kFrames frames / slices of kSlice elements, then the partials in ascending order), so they are bitwise repeatable and
// item b's result is the same whatever else is in the batch (the pattern of reduce.hip / ldm_loss_forward).
#include "common.h"

#include <cfloat>

namespace ldm {
namespace {

constexpr int kFrames = 128;    // frames per block of the MFCC moments
constexpr int kMaxMfcc = 32;
constexpr int kPitch = kMaxMfcc + 1;   // a frame's row in LDS: {1, c_0 .. c_31}
constexpr int kSlice = 4096;    // elements per block of the pair sums
constexpr int kThreads = 256;

#pragma clang fp contract(off)

// block (64), grid (ceil(T / 64), B): one lane per frame, the mel bins in ascending order
__global__ __launch_bounds__(64) void onset_strength_kernel(const float* __restrict__ db, float* __restrict__ env,
                                                            int n_mels, int T, int lag) {
    const int t = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y;
    if (t >= T) return;
    float acc = 0.f;
    if (t >= lag) {
        const float* p = db + (int64_t)b * n_mels * T + t;
#pragma unroll 8
        for (int m = 0; m < n_mels; ++m) {
            const float d = p[(int64_t)m * T] - p[(int64_t)m * T - lag];
            acc = acc + fmaxf(d, 0.f);
        }
        acc = acc / (float)n_mels;
    }
    env[(int64_t)b * T + t] = acc;
}

// acc[c] += lo, acc[(c + 1) % 12] += hi for a class c that is uniform over the wave: a scalar branch to one of twelve
// bodies with constant indices, so the accumulators stay in registers
__device__ __forceinline__ void chroma_add(float (&acc)[12], int c, float lo, float hi) {
    switch (c) {
#define LDM_CHROMA_CASE(K)                       \
    case K:                                      \
        acc[K] = acc[K] + lo;                    \
        acc[(K + 1) % 12] = acc[(K + 1) % 12] + hi; \
        break;
        LDM_CHROMA_CASE(0) LDM_CHROMA_CASE(1) LDM_CHROMA_CASE(2) LDM_CHROMA_CASE(3) LDM_CHROMA_CASE(4)
        LDM_CHROMA_CASE(5) LDM_CHROMA_CASE(6) LDM_CHROMA_CASE(7) LDM_CHROMA_CASE(8) LDM_CHROMA_CASE(9)
        LDM_CHROMA_CASE(10) LDM_CHROMA_CASE(11)
#undef LDM_CHROMA_CASE
        default: break;   // out of band (cls < 0); a class above 11 is ignored too
    }
}

// block (64), grid (ceil(T / 64), B): one lane per frame and its 12 accumulators, the bins in ascending order, kU
// loads in flight per lane (a wave walks its F rows alone: 0.121 ms for [1025, 10336], 0.130 ms with 8 in flight; see
// DESIGN.md §7m)
constexpr int kU = 32;
__global__ __launch_bounds__(64) void chroma_kernel(const float* __restrict__ P, const int32_t* __restrict__ cls,
                                                    const float* __restrict__ wt, float* __restrict__ out, int F,
                                                    int T) {
    const int t = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y;
    if (t >= T) return;
    const float* p = P + (int64_t)b * F * T + t;
    float acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0.f;
    int f0 = 0;
    for (; f0 + kU <= F; f0 += kU) {
        float v[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) v[u] = p[(int64_t)(f0 + u) * T];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int c = cls[f0 + u];
            if (c >= 0) {
                const float w = wt[f0 + u];
                chroma_add(acc, c, w * v[u], (1.0f - w) * v[u]);
            }
        }
    }
    for (int f = f0; f < F; ++f) {
        const int c = cls[f];
        if (c >= 0) {
            const float w = wt[f], v = p[(int64_t)f * T];
            chroma_add(acc, c, w * v, (1.0f - w) * v);
        }
    }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 12; ++k) s = s + acc[k] * acc[k];
    const float n = sqrtf(s);
    const bool live = n >= FLT_MIN;   // false for a NaN as well
    float* o = out + (int64_t)b * 12 * T + t;
#pragma unroll
    for (int k = 0; k < 12; ++k) o[(int64_t)k * T] = live ? acc[k] / n : 0.f;
}

// Entry e of a frame's moments is the pair (j, k), j <= k, of the row a = {1, c_0 .. c_{n-1}} in row-major order:
// row 0 is {sum w, sum w c_k}, rows 1 .. n are sum w c_j c_k (j <= k).
__device__ __forceinline__ void moment_pair(int e, int n1, int& j, int& k) {
    j = 0;
    int row = n1;   // entries in row j
    while (e >= row) {
        e -= row;
        --row;
        ++j;
    }
    k = j + e;
}

// block (256), grid (ceil(T / kFrames), B).  Phase 1: thread (frame tl, half h) forms 16 of the frame's coefficients,
// c_k = sum_m D[k, m] db[m, t] with m ascending; D[k, m] is uniform over the wave (scalar loads).  The row {1, c} and
// the frame's weight go to LDS.  Phase 2: thread e owns moment entries e, e + 256, .. and adds the block's frames in
// ascending order.  part [B][blocks][E].
__global__ __launch_bounds__(kThreads) void mfcc_moments_kernel(const float* __restrict__ db,
                                                                const double* __restrict__ D,
                                                                const float* __restrict__ w,
                                                                double* __restrict__ part, int n_mels, int T,
                                                                int n_mfcc) {
    __shared__ double a[kFrames * kPitch];
    __shared__ double wl[kFrames];
    const int blk = blockIdx.x, b = blockIdx.y, t0 = blk * kFrames;
    const int tl = threadIdx.x & (kFrames - 1), kb = uni((int)(threadIdx.x >> 7) * 16), t = t0 + tl;
    double c[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) c[i] = 0.0;
    if (t < T) {
        const float* p = db + (int64_t)b * n_mels * T + t;
        for (int m = 0; m < n_mels; ++m) {
            const double x = (double)p[(int64_t)m * T];
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (kb + i < n_mfcc) c[i] = fma(D[(int64_t)(kb + i) * n_mels + m], x, c[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (kb + i < n_mfcc) a[tl * kPitch + 1 + kb + i] = c[i];
    if (kb == 0) {
        a[tl * kPitch] = 1.0;
        wl[tl] = t < T ? (w ? (double)w[(int64_t)b * T + t] : 1.0) : 0.0;
    }
    __syncthreads();
    const int n1 = n_mfcc + 1, E = n1 * (n1 + 1) / 2;
    const int nt = T - t0 < kFrames ? T - t0 : kFrames;
    for (int e = threadIdx.x; e < E; e += kThreads) {
        int j, k;
        moment_pair(e, n1, j, k);
        double s = 0.0;
        for (int q = 0; q < nt; ++q) s = fma(wl[q] * a[q * kPitch + j], a[q * kPitch + k], s);
        part[((int64_t)b * gridDim.x + blk) * E + e] = s;
    }
}

// thread stride -> wave shuffle tree -> waves in order (reduce.hip's block_sum)
__device__ __forceinline__ double block_sum(double v, double* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double s = 0.0;
    for (int i = 0; i < kThreads / 64; ++i) s += red[i];
    return s;
}

// block (256), grid (ceil(n / kSlice), B); part [B][slices][7]
__global__ __launch_bounds__(kThreads) void pair_stats_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                              const float* __restrict__ w, double* __restrict__ part,
                                                              int64_t n) {
    __shared__ double red[kThreads / 64];
    const int blk = blockIdx.x, item = blockIdx.y;
    const int64_t base = (int64_t)item * n, e0 = (int64_t)blk * kSlice, e1 = e0 + kSlice < n ? e0 + kSlice : n;
    double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t i = e0 + threadIdx.x; i < e1; i += kThreads) {
        const double x = (double)a[base + i], y = (double)b[base + i], ww = w ? (double)w[base + i] : 1.0;
        const double wa = ww * x, wb = ww * y, d = x - y;   // a product of two fp32 values is exact in float64
        s[0] += ww;
        s[1] += wa;
        s[2] += wb;
        s[3] = fma(wa, x, s[3]);
        s[4] = fma(wb, y, s[4]);
        s[5] = fma(wa, y, s[5]);
        s[6] = fma(ww * d, d, s[6]);
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const double v = block_sum(s[j], red);
        if (threadIdx.x == 0) part[((int64_t)item * gridDim.x + blk) * 7 + j] = v;
    }
}

// out[b][e] = sum_p part[b][p][e], the partials in ascending order.  block (256), grid (ceil(E / 256), B)
__global__ __launch_bounds__(kThreads) void sum_partials_kernel(const double* __restrict__ part, int np, int E,
                                                                double* __restrict__ out) {
    const int e = blockIdx.x * kThreads + threadIdx.x, b = blockIdx.y;
    if (e >= E) return;
    double s = 0.0;
    for (int p = 0; p < np; ++p) s += part[((int64_t)b * np + p) * E + e];
    out[(int64_t)b * E + e] = s;
}

inline int moment_entries(int n_mfcc) { return (n_mfcc + 1) * (n_mfcc + 2) / 2; }

}  // namespace
}  // namespace ldm

using namespace ldm;

extern "C" int ldm_onset_strength(const float* db, int32_t B, int32_t n_mels, int32_t T, int32_t lag, float* env,
                                  void* stream) {
    LDM_REQUIRE(db && env, "onset_strength: null pointer");
    LDM_REQUIRE(B >= 1 && B <= 65535 && n_mels >= 1 && T >= 1, "onset_strength: bad shape (B 1..65535, n_mels, T >= 1)");
    LDM_REQUIRE(lag >= 1, "onset_strength: lag must be at least 1");
    hipLaunchKernelGGL(onset_strength_kernel, dim3((T + 63) / 64, B), dim3(64), 0, (hipStream_t)stream, db, env, n_mels,
                       T, lag);
    LDM_CHECK_LAUNCH("onset_strength_kernel");
    return 0;
}

extern "C" int ldm_chroma(const float* P, const int32_t* cls, const float* wt, int32_t B, int32_t F, int32_t T,
                          float* chroma, void* stream) {
    LDM_REQUIRE(P && cls && wt && chroma, "chroma: null pointer");
    LDM_REQUIRE(B >= 1 && B <= 65535 && F >= 1 && T >= 1, "chroma: bad shape (B 1..65535, F, T >= 1)");
    hipLaunchKernelGGL(chroma_kernel, dim3((T + 63) / 64, B), dim3(64), 0, (hipStream_t)stream, P, cls, wt, chroma, F,
                       T);
    LDM_CHECK_LAUNCH("chroma_kernel");
    return 0;
}

extern "C" int64_t ldm_mfcc_moments_workspace(int32_t B, int32_t T, int32_t n_mfcc) {
    if (B < 1 || T < 1 || n_mfcc < 1 || n_mfcc > kMaxMfcc) return 0;
    return (int64_t)B * ((T + kFrames - 1) / kFrames) * moment_entries(n_mfcc);
}

extern "C" int ldm_mfcc_moments(const float* db, const double* D, const float* w, int32_t B, int32_t n_mels, int32_t T,
                                int32_t n_mfcc, double* mom, double* workspace, void* stream) {
    LDM_REQUIRE(db && D && mom && workspace, "mfcc_moments: null pointer");
    LDM_REQUIRE(n_mfcc >= 1 && n_mfcc <= kMaxMfcc, "mfcc_moments: n_mfcc must lie in 1..32");
    LDM_REQUIRE(B >= 1 && B <= 65535 && n_mels >= 1 && T >= 1, "mfcc_moments: bad shape (B 1..65535, n_mels, T >= 1)");
    LDM_REQUIRE(((uintptr_t)D & 7) == 0 && ((uintptr_t)mom & 7) == 0 && ((uintptr_t)workspace & 7) == 0,
                "mfcc_moments: D, mom and workspace must be 8-byte aligned");
    const int nb = (T + kFrames - 1) / kFrames, E = moment_entries(n_mfcc);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mfcc_moments_kernel, dim3(nb, B), dim3(kThreads), 0, s, db, D, w, workspace, n_mels, T, n_mfcc);
    LDM_CHECK_LAUNCH("mfcc_moments_kernel");
    hipLaunchKernelGGL(sum_partials_kernel, dim3((E + kThreads - 1) / kThreads, B), dim3(kThreads), 0, s, workspace, nb,
                       E, mom);
    LDM_CHECK_LAUNCH("sum_partials_kernel");
    return 0;
}

extern "C" int64_t ldm_pair_stats_workspace(int32_t B, int64_t n) {
    if (B < 1 || n < 1) return 0;
    return (int64_t)B * ((n + kSlice - 1) / kSlice) * 7;
}

extern "C" int ldm_pair_stats(const float* a, const float* b, const float* w, int32_t B, int64_t n, double* out,
                              double* workspace, void* stream) {
    LDM_REQUIRE(a && b && out && workspace, "pair_stats: null pointer");
    LDM_REQUIRE(B >= 1 && B <= 65535 && n >= 1 && n <= ((int64_t)1 << 40), "pair_stats: bad shape (B 1..65535, n 1..2^40)");
    LDM_REQUIRE(((uintptr_t)out & 7) == 0 && ((uintptr_t)workspace & 7) == 0,
                "pair_stats: out and workspace must be 8-byte aligned");
    const int64_t np = (n + kSlice - 1) / kSlice;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pair_stats_kernel, dim3((unsigned)np, B), dim3(kThreads), 0, s, a, b, w, workspace, n);
    LDM_CHECK_LAUNCH("pair_stats_kernel");
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1, B), dim3(kThreads), 0, s, workspace, (int)np, 7, out);
    LDM_CHECK_LAUNCH("sum_partials_kernel");
    return 0;
}
