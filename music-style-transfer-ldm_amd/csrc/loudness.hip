// Loudness: an ITU-R BS.1770-4 / EBU R128 integrated-loudness meter, a 4x-oversampled true-peak meter
// and a look-ahead true-peak limiter for mono fp32 recordings x [B, L]; rows are independent.
//
// Meter.  The K-weighting is two biquads (a shelf, then a high-pass) run in float64 as transposed direct form II, the
// form scipy.signal.sosfilt runs, so the cascade's state is 4 doubles.  The recursion is sequential in time, so it is
// cut into chunks of one hop (round(0.1 sr) samples), one lane per chunk:
//   1. kw_hop_kernel<false>: every chunk runs the cascade from a zero state and stores its end state p_k;
//   2. kw_carry_kernel: one lane per row walks s_{k+1} = M s_k + p_k, M = the 4x4 transition of `hop` zero-input
//      samples (formed once on the host by running the same recursion on the unit states), and replaces p_k by the true
//      start state s_k; the states pass through LDS in runs of 64 so the global traffic is coalesced;
//   3. kw_hop_kernel<true>: every chunk reruns from s_k and adds y^2 in sample order: one float64 sum per hop.
// The filtered signal is never written.  A lane's 2 dependent FMAs per sample and stage are the critical path; a
// 5-minute recording is ~3000 lanes of 2205 samples.  Every hop sum is one lane's sum in sample order, so the result is
// bitwise repeatable and does not depend on B.  loud_gate_kernel: one block per row, the two gates of BS.1770 on the
// 400 ms blocks (4 hops, 75 % overlap), fixed-order float64 block sums, no host synchronisation.
//
// True peak.  tp_kernel: a tile of samples plus a halo of W in LDS, each lane the four oversampling phases of its
// samples with resample.hip's sum (ascending j, one fmaf per tap: bitwise ldm_resample_f32's outputs) and the running
// maximum of |x| and the four |phases|; the 4x signal is never written.  Block maxima, then one block per row.
//
// Limiter.  limit_kernel: one block owns kLimTile samples and holds in LDS the input with a halo of 2 Lh + W, the
// true-peak gain r = min(1, c / p) with a halo of 2 Lh, its running minimum m over |j| <= Lh with a halo of Lh, the
// Hann weights and the taps; g = 1 - sum_j w_j (1 - m[n + j]) and y = g x.  The gain curve never leaves the chip
// unless the caller asks for it.  A tile in which no r is below 1 stores x itself (g is exactly 1 there anyway).
#include "common.h"

#include <cmath>

namespace ldm {
namespace {

constexpr int kThreads = 256;
constexpr int kTpTile = 2048;       // samples per block of the true-peak meter
constexpr int kLimTile = 8192;      // samples per block of the limiter
constexpr int kLimThreads = 1024;
constexpr int kLdsFloats = 160 * 1024 / 4;
constexpr int kLimState = 32;       // floats of block state (wave minima, the any-below-ceiling flag) ahead of the arrays
constexpr int kMaxW = 256;          // half-width of the oversampling filter the kernels take

struct Sos {   // the two sections, a0 = 1: {b0, b1, b2, a1, a2} of the shelf, then of the high-pass
    double b0, b1, b2, a1, a2, c0, c1, c2, d1, d2;
};
struct Mat4 {
    double m[16];   // row-major
};

// one sample through the cascade (transposed direct form II); s = {shelf s1, s2, high-pass s1, s2}
__host__ __device__ __forceinline__ double kw_step(const Sos& q, double x, double (&s)[4]) {
    const double y1 = fma(q.b0, x, s[0]);
    s[0] = fma(-q.a1, y1, fma(q.b1, x, s[1]));
    s[1] = fma(-q.a2, y1, q.b2 * x);
    const double y2 = fma(q.c0, y1, s[2]);
    s[2] = fma(-q.d1, y2, fma(q.c1, y1, s[3]));
    s[3] = fma(-q.d2, y2, q.c2 * y1);
    return y2;
}

// block (64), grid (ceil(nh / 64), B): lane = hop h of row b.  st [B][nh][4]; out [B][nh]
template <bool FINAL>
__global__ __launch_bounds__(64) void kw_hop_kernel(const float* __restrict__ x, int64_t L, int hop, int nh, Sos q,
                                                    double* __restrict__ st, double* __restrict__ out) {
    const int h = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y;
    if (h >= nh) return;
    const float* p = x + (int64_t)b * L + (int64_t)h * hop;
    double* sp = st + ((int64_t)b * nh + h) * 4;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (FINAL) {
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = sp[i];
    }
    double acc = 0.0;
#pragma unroll 4
    for (int n = 0; n < hop; ++n) {
        const double y = kw_step(q, (double)p[n], s);
        if (FINAL) acc = fma(y, y, acc);
    }
    if (FINAL) {
        out[(int64_t)b * nh + h] = acc;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) sp[i] = s[i];
    }
}

// block (64), grid (B): st[b][k] = the zero-state end of chunk k on entry, the true start state of chunk k on exit
__global__ __launch_bounds__(64) void kw_carry_kernel(double* __restrict__ st, int nh, Mat4 M) {
    __shared__ double sp[64 * 4];
    double* s = st + (int64_t)blockIdx.x * nh * 4;
    double c[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < nh; k0 += 64) {
        const int n = nh - k0 < 64 ? nh - k0 : 64;
        for (int i = threadIdx.x; i < n * 4; i += 64) sp[i] = s[(int64_t)k0 * 4 + i];
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int k = 0; k < n; ++k) {
                double p[4], t[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) p[i] = sp[4 * k + i], sp[4 * k + i] = c[i];
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    t[i] = fma(M.m[4 * i + 3], c[3], fma(M.m[4 * i + 2], c[2], fma(M.m[4 * i + 1], c[1],
                                                                                  fma(M.m[4 * i], c[0], p[i]))));
#pragma unroll
                for (int i = 0; i < 4; ++i) c[i] = t[i];
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < n * 4; i += 64) s[(int64_t)k0 * 4 + i] = sp[i];
        __syncthreads();
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

// block (256), grid (B).  hs [B][nh] -> out [B][4] = {integrated LUFS, blocks passing both gates, relative threshold,
// blocks in all}
__global__ __launch_bounds__(kThreads) void loud_gate_kernel(const double* __restrict__ hs, int nh, int hop,
                                                             double* __restrict__ out) {
    __shared__ double red[kThreads / 64];
    const double* h = hs + (int64_t)blockIdx.x * nh;
    const int nb = nh >= 4 ? nh - 3 : 0;
    const double inv = 1.0 / (4.0 * (double)hop), ninf = -INFINITY;
    double sa = 0.0, ca = 0.0;
    for (int j = threadIdx.x; j < nb; j += kThreads) {
        const double z = (((h[j] + h[j + 1]) + h[j + 2]) + h[j + 3]) * inv;
        if (-0.691 + 10.0 * log10(z) > -70.0) sa += z, ca += 1.0;
    }
    sa = block_sum(sa, red);
    ca = block_sum(ca, red);
    double thr = ninf, sb = 0.0, cb = 0.0;
    if (ca > 0.0) {   // uniform over the block
        thr = -0.691 + 10.0 * log10(sa / ca) - 10.0;
        for (int j = threadIdx.x; j < nb; j += kThreads) {
            const double z = (((h[j] + h[j + 1]) + h[j + 2]) + h[j + 3]) * inv;
            const double l = -0.691 + 10.0 * log10(z);
            if (l > -70.0 && l > thr) sb += z, cb += 1.0;
        }
    }
    sb = block_sum(sb, red);
    cb = block_sum(cb, red);
    if (threadIdx.x == 0) {
        double* o = out + (int64_t)blockIdx.x * 4;
        o[0] = cb > 0.0 ? -0.691 + 10.0 * log10(sb / cb) : ninf;
        o[1] = cb;
        o[2] = thr;
        o[3] = (double)nb;
    }
}

// the four oversampling phases at the sample whose window starts at xs[0] (xs[W] is the sample itself): resample.hip's
// sum, ascending j; returns max(|x|, |phase k|)
__device__ __forceinline__ float true_peak_at(const float* xs, const float* st, int K, int W) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int j = 0; j < K; ++j) {
        const float v = xs[j];
        a0 = fmaf(v, st[j], a0);
        a1 = fmaf(v, st[K + j], a1);
        a2 = fmaf(v, st[2 * K + j], a2);
        a3 = fmaf(v, st[3 * K + j], a3);
    }
    return fmaxf(fmaxf(fabsf(xs[W]), fmaxf(fabsf(a0), fabsf(a1))), fmaxf(fabsf(a2), fabsf(a3)));
}

// the block's maximum (MIN: minimum) of v, valid in thread 0
template <bool MIN>
__device__ __forceinline__ float block_extreme(float v, float* red, int nwaves) {
    for (int o = 32; o > 0; o >>= 1) {
        const float u = __shfl_xor(v, o);
        v = MIN ? fminf(v, u) : fmaxf(v, u);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float s = red[0];
    for (int i = 1; i < nwaves; ++i) s = MIN ? fminf(s, red[i]) : fmaxf(s, red[i]);
    return s;
}

// block (256), grid (ceil(L / kTpTile), B), dynamic LDS (kTpTile + 2W + 4K) floats.  part [B][gridDim.x]
__global__ __launch_bounds__(kThreads) void tp_kernel(const float* __restrict__ x, int64_t L,
                                                      const float* __restrict__ taps, int W,
                                                      float* __restrict__ part) {
    extern __shared__ float smem[];
    __shared__ float red[kThreads / 64];
    const int K = 2 * W + 1, nx = kTpTile + 2 * W, b = blockIdx.y;
    float* sx = smem;
    float* st = smem + nx;
    const int64_t t0 = (int64_t)blockIdx.x * kTpTile;
    const float* xb = x + (int64_t)b * L;
    for (int i = threadIdx.x; i < nx; i += kThreads) {
        const int64_t g = t0 - W + i;
        sx[i] = (g >= 0 && g < L) ? xb[g] : 0.f;
    }
    for (int i = threadIdx.x; i < 4 * K; i += kThreads) st[i] = taps[i];
    __syncthreads();
    const int nt = L - t0 < kTpTile ? (int)(L - t0) : kTpTile;
    float mx = 0.f;
    for (int i = threadIdx.x; i < nt; i += kThreads) mx = fmaxf(mx, true_peak_at(sx + i, st, K, W));
    mx = block_extreme<false>(mx, red, kThreads / 64);
    if (threadIdx.x == 0) part[(int64_t)b * gridDim.x + blockIdx.x] = mx;
}

// block (256), grid (B): out[b] = max (MIN: min) of part[b][0 .. np)
template <bool MIN>
__global__ __launch_bounds__(kThreads) void row_extreme_kernel(const float* __restrict__ part, int64_t np,
                                                               float* __restrict__ out) {
    __shared__ float red[kThreads / 64];
    const float* p = part + (int64_t)blockIdx.x * np;
    float v = MIN ? INFINITY : 0.f;
    for (int64_t i = threadIdx.x; i < np; i += kThreads) v = MIN ? fminf(v, p[i]) : fmaxf(v, p[i]);
    v = block_extreme<MIN>(v, red, kThreads / 64);
    if (threadIdx.x == 0) out[blockIdx.x] = v;
}

// block (1024), grid (ceil(L / kLimTile), B), dynamic LDS (kLimState + 3 kLimTile + 12 Lh + 2W + 1 + 4K) floats.
// y, gain [B][L] (gain may be null); gmin [B][gridDim.x] (may be null): the tile's smallest gain
__global__ __launch_bounds__(kLimThreads) void limit_kernel(const float* __restrict__ x, int64_t L,
                                                            const float* __restrict__ taps, int W, int Lh, float c,
                                                            float* __restrict__ y, float* __restrict__ gain,
                                                            float* __restrict__ gmin) {
    extern __shared__ float smem[];   // all of the block's LDS is dynamic: the launch asks for the whole 160 KiB
    float* red = smem;       // kLimThreads / 64 wave minima
    int& s_any = *reinterpret_cast<int*>(smem + kLimThreads / 64);
    const int K = 2 * W + 1, H2 = 2 * Lh, nx = kLimTile + 2 * H2 + 2 * W, nr = kLimTile + 2 * H2, nm = kLimTile + H2;
    float* sx = smem + kLimState;   // sample t0 - 2 Lh - W + i
    float* sr = sx + nx;     // sample t0 - 2 Lh + i
    float* sm = sr + nr;     // sample t0 - Lh + i
    float* sw = sm + nm;     // 2 Lh + 1 Hann weights
    float* st = sw + H2 + 1; // taps [4][K]
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * kLimTile;
    const float* xb = x + (int64_t)b * L;
    if (tid == 0) s_any = 0;
    for (int i = tid; i < nx; i += kLimThreads) {
        const int64_t g = t0 - H2 - W + i;
        sx[i] = (g >= 0 && g < L) ? xb[g] : 0.f;
    }
    for (int i = tid; i < 4 * K; i += kLimThreads) st[i] = taps[i];
    // the 2 Lh + 1 non-zero points of a Hann window of 2 Lh + 3, which sum to Lh + 1
    for (int j = tid; j <= H2; j += kLimThreads)
        sw[j] = (float)((0.5 - 0.5 * cos(M_PI * (double)(j + 1) / (double)(Lh + 1))) / (double)(Lh + 1));
    __syncthreads();
    // r = min(1, c / p) inside [0, L), 1 outside
    bool any = false;
    for (int i = tid; i < nr; i += kLimThreads) {
        const int64_t n = t0 - H2 + i;
        float r = 1.f;
        if (n >= 0 && n < L) {
            const float p = true_peak_at(sx + i, st, K, W);
            if (p > c) r = c / p, any = true;
        }
        sr[i] = r;
    }
    if (any) s_any = 1;   // every writer stores the same value
    __syncthreads();
    const int nt = L - t0 < kLimTile ? (int)(L - t0) : kLimTile;
    float* yb = y + (int64_t)b * L + t0;
    float* gb = gain ? gain + (int64_t)b * L + t0 : nullptr;
    float lo = 1.f;
    if (s_any) {   // uniform over the block
        for (int i = tid; i < nm; i += kLimThreads) {
            float m = sr[i];
            for (int j = 1; j <= H2; ++j) m = fminf(m, sr[i + j]);
            sm[i] = m;
        }
        __syncthreads();
        for (int i = tid; i < nt; i += kLimThreads) {
            float acc = 0.f;
            for (int j = 0; j <= H2; ++j) acc = fmaf(sw[j], 1.0f - sm[i + j], acc);
            const float g = 1.0f - acc;
            yb[i] = g * sx[i + H2 + W];
            if (gb) gb[i] = g;
            lo = fminf(lo, g);
        }
    } else {
        for (int i = tid; i < nt; i += kLimThreads) {
            yb[i] = sx[i + H2 + W];
            if (gb) gb[i] = 1.0f;
        }
    }
    if (gmin) {
        lo = block_extreme<true>(lo, red, kLimThreads / 64);
        if (tid == 0) gmin[(int64_t)b * gridDim.x + blockIdx.x] = lo;
    }
}

// block (256), grid (ceil(L / 1024), B): y = x 10^((target - I_b) / 20), I_b = stats[b][0]; a row that is not finite
// (silence) gets 0 dB.  gain_db [B] float64
__global__ __launch_bounds__(kThreads) void loud_gain_kernel(const float* __restrict__ x, const double* __restrict__ stats,
                                                             double target, int64_t L, float* __restrict__ y,
                                                             double* __restrict__ gain_db) {
    const int b = blockIdx.y;
    const double I = stats[(int64_t)b * 4];
    const double db = (I == I && fabs(I) != INFINITY) ? target - I : 0.0;
    const float g = (float)pow(10.0, db / 20.0);
    if (blockIdx.x == 0 && threadIdx.x == 0) gain_db[b] = db;
    const int64_t i0 = (int64_t)blockIdx.x * (4 * kThreads) + threadIdx.x;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t i = i0 + r * kThreads;
        if (i < L) y[(int64_t)b * L + i] = g * x[(int64_t)b * L + i];
    }
}

// block (256), grid (ceil(L / 1024), B): y *= s_b in place, s_b = 1 where tp[b] <= c, else (c / tp[b]) * margin
__global__ __launch_bounds__(kThreads) void peak_trim_kernel(float* __restrict__ y, const float* __restrict__ tp, float c,
                                                             float margin, int64_t L, float* __restrict__ trim) {
    const int b = blockIdx.y;
    const float t = tp[b];
    const float s = t > c ? (c / t) * margin : 1.0f;
    if (trim && blockIdx.x == 0 && threadIdx.x == 0) trim[b] = s;
    const int64_t i0 = (int64_t)blockIdx.x * (4 * kThreads) + threadIdx.x;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t i = i0 + r * kThreads;
        if (i < L) y[(int64_t)b * L + i] = s * y[(int64_t)b * L + i];
    }
}

inline bool rows_ok(int32_t B, int64_t L) { return B >= 1 && B <= 65535 && L >= 1 && L <= ((int64_t)1 << 40); }
inline int64_t lim_lds_floats(int W, int Lh) { return kLimState + 3 * (int64_t)kLimTile + 12 * (int64_t)Lh + 2 * W + 1 + 4 * (2 * W + 1); }

}  // namespace
}  // namespace ldm

using namespace ldm;

extern "C" int32_t ldm_loudness_chunk(int32_t hop) { return hop >= 1 ? hop : 0; }

extern "C" int64_t ldm_loudness_workspace(int32_t B, int64_t L, int32_t hop) {
    if (!rows_ok(B, L) || hop < 1) return 0;
    return (int64_t)B * (L / hop) * 4;
}

extern "C" int ldm_loudness_hop_sums(const float* x, int32_t B, int64_t L, int32_t hop, const double* sos,
                                     double* hop_sums, double* workspace, void* stream) {
    LDM_REQUIRE(x && sos, "loudness_hop_sums: null pointer");
    LDM_REQUIRE(rows_ok(B, L), "loudness_hop_sums: bad shape (B 1..65535, L 1..2^40)");
    LDM_REQUIRE(hop >= 1 && L / hop < (1 << 30), "loudness_hop_sums: bad hop");
    for (int i = 0; i < 10; ++i) LDM_REQUIRE(std::isfinite(sos[i]), "loudness_hop_sums: non-finite coefficient");
    const int nh = (int)(L / hop);
    if (nh == 0) return 0;   // shorter than one hop: nothing to write
    LDM_REQUIRE(hop_sums && workspace, "loudness_hop_sums: null pointer");
    LDM_REQUIRE(((uintptr_t)hop_sums & 7) == 0 && ((uintptr_t)workspace & 7) == 0,
                "loudness_hop_sums: hop_sums and workspace must be 8-byte aligned");
    const Sos q{sos[0], sos[1], sos[2], sos[3], sos[4], sos[5], sos[6], sos[7], sos[8], sos[9]};
    Mat4 M;   // column i = the state after `hop` zero-input samples from the unit state e_i
    for (int i = 0; i < 4; ++i) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        s[i] = 1.0;
        for (int n = 0; n < hop; ++n) kw_step(q, 0.0, s);
        for (int r = 0; r < 4; ++r) M.m[4 * r + i] = s[r];
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((nh + 63) / 64, B);
    hipLaunchKernelGGL(kw_hop_kernel<false>, grid, dim3(64), 0, st, x, L, hop, nh, q, workspace, hop_sums);
    LDM_CHECK_LAUNCH("kw_hop_kernel<false>");
    hipLaunchKernelGGL(kw_carry_kernel, dim3(B), dim3(64), 0, st, workspace, nh, M);
    LDM_CHECK_LAUNCH("kw_carry_kernel");
    hipLaunchKernelGGL(kw_hop_kernel<true>, grid, dim3(64), 0, st, x, L, hop, nh, q, workspace, hop_sums);
    LDM_CHECK_LAUNCH("kw_hop_kernel<true>");
    return 0;
}

extern "C" int ldm_loudness_gate(const double* hop_sums, int32_t B, int32_t n_hops, int32_t hop, double* out,
                                 void* stream) {
    LDM_REQUIRE(out && (hop_sums || n_hops == 0), "loudness_gate: null pointer");
    LDM_REQUIRE(B >= 1 && B <= 65535 && n_hops >= 0 && hop >= 1, "loudness_gate: bad shape (B 1..65535, n_hops >= 0, hop >= 1)");
    LDM_REQUIRE(((uintptr_t)hop_sums & 7) == 0 && ((uintptr_t)out & 7) == 0,
                "loudness_gate: hop_sums and out must be 8-byte aligned");
    hipLaunchKernelGGL(loud_gate_kernel, dim3(B), dim3(kThreads), 0, (hipStream_t)stream, hop_sums, n_hops, hop, out);
    LDM_CHECK_LAUNCH("loud_gate_kernel");
    return 0;
}

extern "C" int ldm_loudness_gain(const float* x, const double* stats, double target_lufs, int32_t B, int64_t L,
                                 float* y, double* gain_db, void* stream) {
    LDM_REQUIRE(x && stats && y && gain_db, "loudness_gain: null pointer");
    LDM_REQUIRE(rows_ok(B, L), "loudness_gain: bad shape (B 1..65535, L 1..2^40)");
    LDM_REQUIRE(std::isfinite(target_lufs), "loudness_gain: target must be finite");
    const int64_t nb = (L + 4 * kThreads - 1) / (4 * kThreads);
    LDM_REQUIRE(nb <= 0x7fffffff, "loudness_gain: L too long");
    hipLaunchKernelGGL(loud_gain_kernel, dim3((unsigned)nb, B), dim3(kThreads), 0, (hipStream_t)stream, x, stats,
                       target_lufs, L, y, gain_db);
    LDM_CHECK_LAUNCH("loud_gain_kernel");
    return 0;
}

extern "C" int64_t ldm_true_peak_workspace(int32_t B, int64_t L) {
    if (!rows_ok(B, L)) return 0;
    return (int64_t)B * ((L + kTpTile - 1) / kTpTile);
}

extern "C" int ldm_true_peak(const float* x, int32_t B, int64_t L, const float* taps, int32_t up, int32_t W, float* out,
                             float* workspace, void* stream) {
    LDM_REQUIRE(x && taps && out && workspace, "true_peak: null pointer");
    LDM_REQUIRE(rows_ok(B, L), "true_peak: bad shape (B 1..65535, L 1..2^40)");
    LDM_REQUIRE(up == 4 && W >= 0 && W <= kMaxW, "true_peak: the taps must be a [4, 2W+1] table, W <= 256");
    const int64_t np = (L + kTpTile - 1) / kTpTile;
    LDM_REQUIRE(np <= 0x7fffffff, "true_peak: L too long");
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = sizeof(float) * (size_t)(kTpTile + 2 * W + 4 * (2 * W + 1));
    hipLaunchKernelGGL(tp_kernel, dim3((unsigned)np, B), dim3(kThreads), lds, st, x, L, taps, W, workspace);
    LDM_CHECK_LAUNCH("tp_kernel");
    hipLaunchKernelGGL(row_extreme_kernel<false>, dim3(B), dim3(kThreads), 0, st, (const float*)workspace, np, out);
    LDM_CHECK_LAUNCH("row_extreme_kernel");
    return 0;
}

extern "C" int32_t ldm_limit_tile(void) { return kLimTile; }

extern "C" int64_t ldm_limit_workspace(int32_t B, int64_t L) {
    if (!rows_ok(B, L)) return 0;
    return (int64_t)B * ((L + kLimTile - 1) / kLimTile);
}

extern "C" int ldm_limit(const float* x, int32_t B, int64_t L, const float* taps, int32_t up, int32_t W,
                         int32_t lookahead, float ceiling, float* y, float* gain, float* min_gain, float* workspace,
                         void* stream) {
    LDM_REQUIRE(x && taps && y, "limit: null pointer");
    LDM_REQUIRE(!min_gain || workspace, "limit: min_gain needs the workspace");
    LDM_REQUIRE(rows_ok(B, L), "limit: bad shape (B 1..65535, L 1..2^40)");
    LDM_REQUIRE(up == 4 && W >= 0 && W <= kMaxW, "limit: the taps must be a [4, 2W+1] table, W <= 256");
    LDM_REQUIRE(ceiling > 0.f && ceiling <= 1.f, "limit: the ceiling must lie in (0, 1]");
    LDM_REQUIRE(lookahead >= 0, "limit: the lookahead must not be negative");
    LDM_REQUIRE(lim_lds_floats(W, lookahead) <= kLdsFloats,
                "limit: the lookahead exceeds what one tile holds in LDS (LDM_LIMIT_MAX_LOOKAHEAD samples at W = 34)");
    LDM_REQUIRE(x != y && (!gain || (gain != x && gain != y)), "limit: y and gain must not alias x or each other");
    const int64_t np = (L + kLimTile - 1) / kLimTile;
    LDM_REQUIRE(np <= 0x7fffffff, "limit: L too long");
    static bool opted = false;
    if (!opted) {
        LDM_HIP_TRY(hipFuncSetAttribute((const void*)limit_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        kLdsFloats * 4));
        opted = true;
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = sizeof(float) * (size_t)lim_lds_floats(W, lookahead);
    hipLaunchKernelGGL(limit_kernel, dim3((unsigned)np, B), dim3(kLimThreads), lds, st, x, L, taps, W, lookahead, ceiling,
                       y, gain, min_gain ? workspace : nullptr);
    LDM_CHECK_LAUNCH("limit_kernel");
    if (min_gain) {
        hipLaunchKernelGGL(row_extreme_kernel<true>, dim3(B), dim3(kThreads), 0, st, (const float*)workspace, np, min_gain);
        LDM_CHECK_LAUNCH("row_extreme_kernel");
    }
    return 0;
}

extern "C" int ldm_peak_trim(float* y, const float* true_peak, float ceiling, int32_t B, int64_t L, float* trim,
                             void* stream) {
    LDM_REQUIRE(y && true_peak, "peak_trim: null pointer");
    LDM_REQUIRE(rows_ok(B, L), "peak_trim: bad shape (B 1..65535, L 1..2^40)");
    LDM_REQUIRE(ceiling > 0.f && ceiling <= 1.f, "peak_trim: the ceiling must lie in (0, 1]");
    const int64_t nb = (L + 4 * kThreads - 1) / (4 * kThreads);
    LDM_REQUIRE(nb <= 0x7fffffff, "peak_trim: L too long");
    hipLaunchKernelGGL(peak_trim_kernel, dim3((unsigned)nb, B), dim3(kThreads), 0, (hipStream_t)stream, y, true_peak,
                       ceiling, 1.0f - 0x1p-15f, L, trim);
    LDM_CHECK_LAUNCH("peak_trim_kernel");
    return 0;
}
