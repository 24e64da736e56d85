// The audio side of the path (DESIGN.md "Audio front and back end"): STFT / ISTFT with librosa's defaults
// (periodic Hann, hop = n_fft/4, centre reflect padding), the fused Griffin-Lim loop, the Slaney mel
// projection, power <-> dB and the projected-gradient mel inversion.  All fp32 (power spectra span 8 decades).
//
// Transforms: a real n_fft-point frame is packed as H = n_fft/2 complex points z[n] = x[2n] + i x[2n+1], transformed
// by an in-LDS radix-4 FFT (H = 4^4 or 4^5: 4 or 5 passes, H/4 lanes per frame) and split into the n_fft/2+1 bins.
// Forward = decimation in frequency (natural in, base-4 digit-reversed out), inverse = its transpose (decimation in
// time, digit-reversed in, natural out), so neither needs a reorder pass or a second buffer.  Twiddles and the window
// come from a table the host builds in float64 (ldm_stft_fill_tables).
//
// LDS: re / im in separate float arrays, element i at sw(i) = i ^ f(bit5, bit6).  A pass of stride s = 4^q has the
// 32 lanes of a bank group vary index bits {0..2q-1} u {2q+2..6}; the XOR makes the five bank bits a full-rank map of
// each of those sets, so every butterfly load / store of every pass is conflict-free (ds_read_b32 / ds_write_b32:
// 32 banks per 32-lane half).  The split step reads Z[k] and Z[H-k] through the digit reversal and is not.
//
// Global layout is [B, F, T] (T contiguous) while a frame yields F contiguous: a workgroup transforms 4 neighbouring
// frames into an LDS tile [4][H+8] of float2 and stores / loads it with t fastest (32-byte runs; H+8 = 8 mod 32
// keeps the four frames' ds_read_b64 on disjoint banks).
#include "common.h"
#include "mel_db.h"

#include <cmath>
#include <type_traits>
#include <vector>

namespace ldm {
namespace {

constexpr int kFrames = 4;     // frames per LDS tile
constexpr int kThreads = 256;
constexpr float kTiny = 1.17549435e-38f;   // smallest normal fp32

__device__ __forceinline__ int sw(int i) { return i ^ (((i >> 5) & 1) * 5) ^ (((i >> 6) & 1) * 26); }

// position of bin k after the forward passes: base-4 digit reversal over P digits
template <int P>
__device__ __forceinline__ int drev(int k) {
    int r = 0;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        r = (r << 2) | (k & 3);
        k >>= 2;
    }
    return r;
}

// Table layout (floats), H = n_fft/2:  [0, 2H) exp(-2 pi i k / H), k < H;  [2H, 4H+2) exp(-2 pi i k / n_fft), k <= H;
// [4H+2, 4H+2+n_fft) the periodic Hann window.
__host__ __device__ constexpr int64_t table_floats(int n_fft) { return 2 * (int64_t)n_fft + 2 + n_fft; }

template <int LOG2N>
struct Geo {
    static constexpr int N = 1 << LOG2N;
    static constexpr int H = N / 2;
    static constexpr int P = (LOG2N - 1) / 2;          // radix-4 passes
    static constexpr int NT = H / 4;                   // lanes per frame
    static constexpr int G = kThreads / NT;            // frames transformed at once (1 or 4)
    static constexpr int HOP = N / 4;
    static constexpr int FP = H + 8;                   // tile row pitch (float2)
    static_assert((LOG2N - 1) % 2 == 0 && NT <= kThreads && kFrames % G == 0, "n_fft/2 must be a power of 4");
};

// forward passes on one frame's re / im (swizzled), lane j of NT.  Ends with a barrier.
template <int LOG2N>
__device__ __forceinline__ void fft_forward(float* re, float* im, const float2* __restrict__ twH, int j) {
    using X = Geo<LOG2N>;
#pragma unroll
    for (int p = 0; p < X::P; ++p) {
        const int s = X::H >> (2 * (p + 1));
        const int r = j & (s - 1);
        const int base = ((j - r) << 2) + r;
        float ar[4], ai[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int a = sw(base + m * s);
            ar[m] = re[a];
            ai[m] = im[a];
        }
        const float b0r = ar[0] + ar[2], b0i = ai[0] + ai[2];
        const float b1r = ar[0] - ar[2], b1i = ai[0] - ai[2];
        const float b2r = ar[1] + ar[3], b2i = ai[1] + ai[3];
        const float b3r = ai[1] - ai[3], b3i = -(ar[1] - ar[3]);   // -i (a1 - a3)
        float yr[4] = {b0r + b2r, b1r + b3r, b0r - b2r, b1r - b3r};
        float yi[4] = {b0i + b2i, b1i + b3i, b0i - b2i, b1i - b3i};
        const int tstep = r * (X::H / (4 * s));   // w_{4s}^{r m} = twH[r m H / 4s]
        {
            const int a = sw(base);
            re[a] = yr[0];
            im[a] = yi[0];
        }
#pragma unroll
        for (int m = 1; m < 4; ++m) {
            const float2 w = twH[tstep * m];
            const int a = sw(base + m * s);
            re[a] = yr[m] * w.x - yi[m] * w.y;
            im[a] = yr[m] * w.y + yi[m] * w.x;
        }
        __syncthreads();
    }
}

// inverse passes (unscaled): input at digit-reversed positions, output natural.  Ends with a barrier.
template <int LOG2N>
__device__ __forceinline__ void fft_inverse(float* re, float* im, const float2* __restrict__ twH, int j) {
    using X = Geo<LOG2N>;
#pragma unroll
    for (int p = X::P - 1; p >= 0; --p) {
        const int s = X::H >> (2 * (p + 1));
        const int r = j & (s - 1);
        const int base = ((j - r) << 2) + r;
        const int tstep = r * (X::H / (4 * s));
        float ar[4], ai[4];
        {
            const int a = sw(base);
            ar[0] = re[a];
            ai[0] = im[a];
        }
#pragma unroll
        for (int m = 1; m < 4; ++m) {
            const float2 w = twH[tstep * m];   // conjugated below
            const int a = sw(base + m * s);
            const float xr = re[a], xi = im[a];
            ar[m] = xr * w.x + xi * w.y;
            ai[m] = xi * w.x - xr * w.y;
        }
        const float b0r = ar[0] + ar[2], b0i = ai[0] + ai[2];
        const float b1r = ar[0] - ar[2], b1i = ai[0] - ai[2];
        const float b2r = ar[1] + ar[3], b2i = ai[1] + ai[3];
        const float b3r = -(ai[1] - ai[3]), b3i = ar[1] - ar[3];   // +i (a1 - a3)
        const float yr[4] = {b0r + b2r, b1r + b3r, b0r - b2r, b1r - b3r};
        const float yi[4] = {b0i + b2i, b1i + b3i, b0i - b2i, b1i - b3i};
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int a = sw(base + m * s);
            re[a] = yr[m];
            im[a] = yi[m];
        }
        __syncthreads();
    }
}

struct StftOut {
    float2* S;         // [B, F, T] complex, or null
    float* mag;        // [B, F, T] |S|^power, or null
    int power;         // 1 or 2
    float2* r_prev;    // Griffin-Lim: previous rebuilt spectrum (read, then overwritten with this one), or null
    float2* angles;    // Griffin-Lim: unit phase of  r - mom * r_prev
    float mom;         // momentum / (1 + momentum)
};

// The anchored Griffin-Lim epilogue's two extra operands: the phase the loop is pulled towards and
// how strongly, per bin.
struct StftOutAnchored : StftOut {
    const float2* p0;   // [B, F, T] unit phase
    const float* aw;    // [B, F, T] weight in [0, 1]
};
template <bool ANCHOR>
using StftOutOf = std::conditional_t<ANCHOR, StftOutAnchored, StftOut>;

// grid (ceil(T / 4), B).  y [B, L]; frame t covers y_padded[t hop, t hop + N), y_padded = reflect pad by N/2.
// ANCHOR: the Griffin-Lim epilogue stores unit(a p0 + (1 - a) angles) instead of angles: angles itself where a == 0
// and p0 itself where a == 1, bitwise (p0 is read only where a > 0).
template <int LOG2N, bool ANCHOR = false>
__global__ __launch_bounds__(kThreads) void stft_kernel(const float* __restrict__ y, int64_t L, int T,
                                                        const float* __restrict__ tables, StftOutOf<ANCHOR> o) {
    using X = Geo<LOG2N>;
    constexpr int N = X::N, H = X::H, NT = X::NT, G = X::G, F = H + 1;
    __shared__ float s_re[G * H];
    __shared__ float s_im[G * H];
    __shared__ float2 s_tile[kFrames * X::FP];
    const float2* twH = reinterpret_cast<const float2*>(tables);
    const float2* twN = reinterpret_cast<const float2*>(tables + 2 * H);
    const float* win = tables + 4 * H + 2;
    const int b = blockIdx.y, t0 = blockIdx.x * kFrames;
    const int g = threadIdx.x / NT, j = threadIdx.x % NT;
    const float* yb = y + (int64_t)b * L;
    float* re = s_re + g * H;
    float* im = s_im + g * H;

    for (int f0 = 0; f0 < kFrames; f0 += G) {
        const int f = f0 + g;
        // frames past T transform the clamped frame T-1 (kept uniform for the barriers; never stored)
        const int t = min(t0 + f, T - 1);
        const int64_t start = (int64_t)t * X::HOP - N / 2;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int n = j + m * NT;
            int64_t i0 = start + 2 * n, i1 = i0 + 1;
            i0 = i0 < 0 ? -i0 : (i0 >= L ? 2 * (L - 1) - i0 : i0);
            i1 = i1 < 0 ? -i1 : (i1 >= L ? 2 * (L - 1) - i1 : i1);
            const int a = sw(n);
            re[a] = yb[i0] * win[2 * n];
            im[a] = yb[i1] * win[2 * n + 1];
        }
        __syncthreads();
        fft_forward<LOG2N>(re, im, twH, j);
        // split: X[k] = E[k] + w_N^k O[k],  E = (Z[k] + conj Z[H-k]) / 2,  O = (Z[k] - conj Z[H-k]) / 2i
        float2* row = s_tile + f * X::FP;
        for (int k = j; k <= H; k += NT) {
            const int pa = sw(drev<X::P>(k & (H - 1)));
            const int pb = sw(drev<X::P>((H - k) & (H - 1)));
            const float zr = re[pa], zi = im[pa], cr = re[pb], ci = -im[pb];
            const float er = 0.5f * (zr + cr), ei = 0.5f * (zi + ci);
            const float orr = 0.5f * (zi - ci), oi = -0.5f * (zr - cr);
            const float2 w = twN[k];
            row[k] = make_float2(er + orr * w.x - oi * w.y, ei + orr * w.y + oi * w.x);
        }
        __syncthreads();
    }

    for (int idx = threadIdx.x; idx < F * kFrames; idx += kThreads) {
        const int k = idx / kFrames, f = idx % kFrames, t = t0 + f;
        if (t >= T) continue;
        const float2 v = s_tile[f * X::FP + k];
        const int64_t at = ((int64_t)b * F + k) * T + t;
        if (o.S) o.S[at] = v;
        if (o.mag) {
            const float p2 = v.x * v.x + v.y * v.y;
            o.mag[at] = o.power == 2 ? p2 : sqrtf(p2);
        }
        if (o.angles) {
            const float2 rp = o.r_prev[at];
            const float ax = v.x - o.mom * rp.x, ay = v.y - o.mom * rp.y;
            const float inv = 1.0f / (sqrtf(ax * ax + ay * ay) + kTiny);
            float2 ang = make_float2(ax * inv, ay * inv);
            if constexpr (ANCHOR) {
                const float w = o.aw[at];
                if (w > 0.f) {
                    const float2 p = o.p0[at];
                    if (w >= 1.f) {
                        ang = p;
                    } else {
                        const float bx = w * p.x + (1.0f - w) * ang.x, by = w * p.y + (1.0f - w) * ang.y;
                        const float binv = 1.0f / (sqrtf(bx * bx + by * by) + kTiny);
                        ang = make_float2(bx * binv, by * binv);
                    }
                }
            }
            o.angles[at] = ang;
            o.r_prev[at] = v;
        }
    }
}

// Inverse STFT, overlap-add in gather form.  The padded signal is cut in hop-sized segments; segment j is the sum
// of the windowed quarters of frames j-3 .. j, added in ascending frame order by one lane.  A workgroup owns
// segments [j0, j0 + seg) of one batch item and inverts frames j0-3 .. j0+seg-1 (3 of them shared with its
// neighbour), 4 at a time through the LDS tile, into a ring of hop-sized accumulators; a segment is divided by
// the window sum-of-squares envelope and written once its last frame has been added.  grid (blocks, B).
template <int LOG2N>
__global__ __launch_bounds__(kThreads) void istft_kernel(const float2* __restrict__ S, const float* __restrict__ mag,
                                                         float* __restrict__ y, int64_t L, int T, int jbeg, int jend,
                                                         int seg, const float* __restrict__ tables) {
    using X = Geo<LOG2N>;
    constexpr int N = X::N, H = X::H, NT = X::NT, G = X::G, F = H + 1, HOP = X::HOP;
    constexpr int RING = (G == 1 ? 4 : 8);   // segments alive at once: 3 + G, rounded to a power of two
    __shared__ float s_re[G * H];
    __shared__ float s_im[G * H];
    __shared__ float2 s_tile[kFrames * X::FP];
    __shared__ float s_acc[RING * HOP];
    const float2* twH = reinterpret_cast<const float2*>(tables);
    const float2* twN = reinterpret_cast<const float2*>(tables + 2 * H);
    const float* win = tables + 4 * H + 2;
    const int b = blockIdx.y;
    const int j0 = jbeg + blockIdx.x * seg, j1 = min(j0 + seg, jend);
    const int g = threadIdx.x / NT, j = threadIdx.x % NT;
    float* re = s_re + g * H;
    float* im = s_im + g * H;
    float* yb = y + (int64_t)b * L;

    for (int i = threadIdx.x; i < RING * HOP; i += kThreads) s_acc[i] = 0.f;
    // frames beyond T-1 are empty: they add nothing, but their segment is still flushed
    for (int tc = max(0, j0 - 3); tc < j1; tc += kFrames) {
        __syncthreads();
        for (int idx = threadIdx.x; idx < F * kFrames; idx += kThreads) {
            const int k = idx / kFrames, f = idx % kFrames, t = tc + f;
            float2 v = make_float2(0.f, 0.f);
            if (t < T) {
                const int64_t at = ((int64_t)b * F + k) * T + t;
                v = S[at];
                if (mag) {
                    const float m = mag[at];
                    v.x *= m, v.y *= m;
                }
                if (k == 0 || k == H) v.y = 0.f;   // a real signal's DC and Nyquist bins (as irfft)
            }
            s_tile[f * X::FP + k] = v;
        }
        __syncthreads();
        for (int f0 = 0; f0 < kFrames; f0 += G) {
            const int tg = tc + f0;          // first frame of this group
            if (tg >= j1) break;
            const float2* row = s_tile + (f0 + g) * X::FP;
            // Z[k] = E[k] + i O[k],  E = (X[k] + conj X[H-k]) / 2,  O = (X[k] - conj X[H-k]) / 2 * conj(w_N^k)
            for (int k = j; k < H; k += NT) {
                const float2 xa = row[k], xb = row[H - k];
                const float er = 0.5f * (xa.x + xb.x), ei = 0.5f * (xa.y - xb.y);
                const float dr = 0.5f * (xa.x - xb.x), di = 0.5f * (xa.y + xb.y);
                const float2 w = twN[k];
                const float orr = dr * w.x + di * w.y, oi = di * w.x - dr * w.y;
                const int a = sw(drev<X::P>(k));
                re[a] = er - oi;
                im[a] = ei + orr;
            }
            __syncthreads();
            fft_inverse<LOG2N>(re, im, twH, j);
            // overlap-add, gather form: every lane owns accumulator cells (segment js, offset r) and adds the group's
            // frames that cover them in ascending frame order
            for (int pos = threadIdx.x; pos < (G + 3) * HOP; pos += kThreads) {
                const int js = tg + pos / HOP, r = pos & (HOP - 1);
                float sum = s_acc[(js & (RING - 1)) * HOP + r];
#pragma unroll
                for (int gg = 0; gg < G; ++gg) {
                    const int t = tg + gg, q = js - t;   // frame t's quarter q lies in segment js
                    if (t >= T || q < 0 || q > 3) continue;
                    const int i = q * HOP + r, a = sw(i >> 1);
                    const float v = (i & 1) ? s_im[gg * H + a] : s_re[gg * H + a];
                    sum += v * (win[i] * (1.0f / H));
                }
                s_acc[(js & (RING - 1)) * HOP + r] = sum;
            }
            __syncthreads();
            // segments tg .. tg+G-1 are complete
            for (int i = threadIdx.x; i < G * HOP; i += kThreads) {
                const int js = tg + i / HOP, r = i & (HOP - 1);
                const int slot = js & (RING - 1);
                const float v = s_acc[slot * HOP + r];
                s_acc[slot * HOP + r] = 0.f;
                if (js < j0 || js >= j1) continue;
                const int64_t p = (int64_t)js * HOP + r, n = p - N / 2;
                if (n < 0 || n >= L) continue;
                float env = 0.f;
#pragma unroll
                for (int q = 3; q >= 0; --q) {   // frames js-3 .. js, ascending
                    const int t = js - q;
                    if (t >= 0 && t < T) {
                        const float wq = win[q * HOP + r];
                        env += wq * wq;
                    }
                }
                yb[n] = env > kTiny ? v / env : v;
            }
            __syncthreads();
        }
    }
}

// mel[b, m, t] = sum_{k in [lo_m, hi_m)} M[m, k] P[b, k, t]: one lane per (m, t), t fastest; the filter row and its
// range are uniform over a wave.  block (64, 4), grid (ceil(T/64), ceil(n_mels/4), B)
__global__ __launch_bounds__(256) void mel_project_kernel(const float* __restrict__ P, const float* __restrict__ M,
                                                          const int32_t* __restrict__ lohi, float* __restrict__ mel,
                                                          int F, int n_mels, int T) {
    const int t = blockIdx.x * 64 + threadIdx.x, m = blockIdx.y * 4 + threadIdx.y, b = blockIdx.z;
    if (m >= n_mels || t >= T) return;
    const int lo = lohi[2 * m], hi = lohi[2 * m + 1];
    const float* p = P + (int64_t)b * F * T + t;
    const float* w = M + (int64_t)m * F;
    float acc = 0.f;
    for (int k = lo; k < hi; ++k) acc = fmaf(w[k], p[(int64_t)k * T], acc);
    mel[((int64_t)b * n_mels + m) * T + t] = acc;
}

// per item: ref[b] = 10 log10(max(amin, max x)).  One block per item; max is exact in any order.
__global__ __launch_bounds__(1024) void db_ref_kernel(const float* __restrict__ x, int64_t n, float amin,
                                                      float* __restrict__ ref) {
    __shared__ float s[1024];
    const float* xb = x + (int64_t)blockIdx.x * n;
    float m = -INFINITY;
    for (int64_t i = threadIdx.x; i < n; i += 1024) m = fmaxf(m, xb[i]);
    s[threadIdx.x] = m;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] = fmaxf(s[threadIdx.x], s[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) ref[blockIdx.x] = db_ref(s[0], amin);
}

__global__ __launch_bounds__(256) void power_to_db_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t n,
                                                          float amin, float top_db, const float* __restrict__ ref) {
#pragma clang fp contract(off)   // 10 log10(max) - ref must cancel exactly: the item's maximum is 0 dB (power_db1)
    const int b = blockIdx.y;
    const float r = ref[b];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        out[(int64_t)b * n + i] = power_db1(x[(int64_t)b * n + i], amin, top_db, r);
}

__global__ __launch_bounds__(256) void db_to_power_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = db_power1(x[i]);
}

__global__ __launch_bounds__(256) void sqrt_kernel(float* __restrict__ x, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) x[i] = sqrtf(x[i]);
}

// C[b] = epi(A . X[b]): A [R, K] row-major shared by the batch, X [K, T], C [R, T].  64x64 tile, 16-deep K steps,
// 256 lanes x 4x4.  With `lohi` (per-row [lo, hi) of A's non-zero run) the K loop covers only the tile's rows' runs.
//   EPI 0: C = max(acc, 0)      EPI 1: C = acc - D      EPI 2: C = max(C - acc * scale, 0)
template <int EPI>
__global__ __launch_bounds__(256) void gemm_kernel(const float* __restrict__ A, const float* __restrict__ Xm,
                                                   float* __restrict__ C, const float* __restrict__ D,
                                                   const int32_t* __restrict__ lohi, int R, int K, int T, float scale) {
    __shared__ float sa[16][64 + 4];
    __shared__ float sx[16][64];
    const int b = blockIdx.z, r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
    const float* xb = Xm + (int64_t)b * K * T;
    const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;
    int kbeg = 0, kend = K;
    if (lohi) {
        kbeg = K, kend = 0;
        for (int r = r0; r < min(r0 + 64, R); ++r) kbeg = min(kbeg, lohi[2 * r]), kend = max(kend, lohi[2 * r + 1]);
        kbeg &= ~15;
    }
    float acc[4][4] = {};
    for (int k0 = kbeg; k0 < kend; k0 += 16) {
        for (int i = threadIdx.x; i < 64 * 16; i += 256) {
            const int rr = i / 16, kk = i % 16;   // A: k fastest
            sa[kk][rr] = (r0 + rr < R && k0 + kk < K) ? A[(int64_t)(r0 + rr) * K + k0 + kk] : 0.f;
            const int k2 = i / 64, cc = i % 64;   // X: t fastest
            sx[k2][cc] = (k0 + k2 < K && c0 + cc < T) ? xb[(int64_t)(k0 + k2) * T + c0 + cc] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            float a[4], x[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = sa[kk][ty * 4 + i], x[i] = sx[kk][tx + 16 * i];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[i][q] = fmaf(a[i], x[q], acc[i][q]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = r0 + ty * 4 + i, c = c0 + tx + 16 * q;
            if (r >= R || c >= T) continue;
            const int64_t at = ((int64_t)b * R + r) * T + c;
            if constexpr (EPI == 0) C[at] = fmaxf(acc[i][q], 0.f);
            if constexpr (EPI == 1) C[at] = acc[i][q] - D[at];
            if constexpr (EPI == 2) C[at] = fmaxf(C[at] - acc[i][q] * scale, 0.f);
        }
}

unsigned grid_for(int64_t n) {
    int64_t b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 16384 ? 16384 : b));
}

int launch_stft(const float* y, int B, int64_t L, int n_fft, int T, const float* tables, const StftOut& o, hipStream_t st) {
    const dim3 grid((T + kFrames - 1) / kFrames, B);
    if (n_fft == 2048)
        hipLaunchKernelGGL(stft_kernel<11>, grid, dim3(kThreads), 0, st, y, L, T, tables, o);
    else
        hipLaunchKernelGGL(stft_kernel<9>, grid, dim3(kThreads), 0, st, y, L, T, tables, o);
    LDM_CHECK_LAUNCH("stft_kernel");
    return 0;
}

int launch_stft_anchored(const float* y, int B, int64_t L, int n_fft, int T, const float* tables, const StftOutAnchored& o,
                         hipStream_t st) {
    const dim3 grid((T + kFrames - 1) / kFrames, B);
    if (n_fft == 2048)
        hipLaunchKernelGGL((stft_kernel<11, true>), grid, dim3(kThreads), 0, st, y, L, T, tables, o);
    else
        hipLaunchKernelGGL((stft_kernel<9, true>), grid, dim3(kThreads), 0, st, y, L, T, tables, o);
    LDM_CHECK_LAUNCH("stft_kernel<anchored>");
    return 0;
}

int launch_istft(const float* S, const float* mag, float* y, int B, int T, int64_t L, int n_fft, const float* tables,
                 hipStream_t st) {
    const int hop = n_fft / 4;
    // segments that overlap the kept samples: padded positions [n_fft/2, n_fft/2 + L)
    const int jbeg = 2, jend = (int)((n_fft / 2 + L - 1) / hop) + 1;
    // 9 segments per workgroup: 12 frames inverted for 9 kept (three tiles of 4)
    const int seg = 9;
    const dim3 grid((jend - jbeg + seg - 1) / seg, B);
    if (n_fft == 2048)
        hipLaunchKernelGGL(istft_kernel<11>, grid, dim3(kThreads), 0, st, reinterpret_cast<const float2*>(S), mag, y, L, T,
                           jbeg, jend, seg, tables);
    else
        hipLaunchKernelGGL(istft_kernel<9>, grid, dim3(kThreads), 0, st, reinterpret_cast<const float2*>(S), mag, y, L, T,
                           jbeg, jend, seg, tables);
    LDM_CHECK_LAUNCH("istft_kernel");
    return 0;
}

// The Griffin-Lim loop of ldm_griffinlim / ldm_griffinlim_anchored (p0 and aw null: the plain epilogue).
int run_griffinlim(const float* mag, const float* init_angles, const float* p0, const float* aw, float* y, int B, int T,
                   int64_t L, int n_fft, int n_iter, float momentum, const float* tables, float* workspace,
                   hipStream_t st) {
    const int64_t cplx = 2 * (int64_t)B * (n_fft / 2 + 1) * T;
    float* r_prev = workspace;
    float* angles = workspace + cplx;
    LDM_HIP_TRY(hipMemsetAsync(r_prev, 0, sizeof(float) * cplx, st));
    const float* cur = init_angles;
    for (int it = 0; it < n_iter; ++it) {
        if (int rc = launch_istft(cur, mag, y, B, T, L, n_fft, tables, st)) return rc;
        StftOut o{nullptr, nullptr, 0, reinterpret_cast<float2*>(r_prev), reinterpret_cast<float2*>(angles),
                  momentum / (1.0f + momentum)};
        if (p0) {
            StftOutAnchored oa{o, reinterpret_cast<const float2*>(p0), aw};
            if (int rc = launch_stft_anchored(y, B, L, n_fft, T, tables, oa, st)) return rc;
        } else {
            if (int rc = launch_stft(y, B, L, n_fft, T, tables, o, st)) return rc;
        }
        cur = angles;
    }
    return launch_istft(cur, mag, y, B, T, L, n_fft, tables, st);
}

}  // namespace
}  // namespace ldm

using namespace ldm;

#define LDM_AUDIO_GEOMETRY(what, n_fft, hop)                                                                      \
    LDM_REQUIRE((n_fft) == 512 || (n_fft) == 2048, what ": unsupported n_fft (512 and 2048 are built)");          \
    LDM_REQUIRE((hop) == (n_fft) / 4, what ": hop must be n_fft / 4")

extern "C" int64_t ldm_stft_table_floats(int32_t n_fft) {
    return (n_fft == 512 || n_fft == 2048) ? table_floats(n_fft) : 0;
}

extern "C" int ldm_stft_fill_tables(int32_t n_fft, float* host_tables) {
    LDM_REQUIRE(n_fft == 512 || n_fft == 2048, "stft_fill_tables: unsupported n_fft (512 and 2048 are built)");
    LDM_REQUIRE(host_tables, "stft_fill_tables: null pointer");
    const int H = n_fft / 2;
    const double two_pi = 6.283185307179586476925286766559;
    float* p = host_tables;
    for (int k = 0; k < H; ++k) {
        *p++ = (float)std::cos(two_pi * k / H);
        *p++ = (float)-std::sin(two_pi * k / H);
    }
    for (int k = 0; k <= H; ++k) {
        *p++ = (float)std::cos(two_pi * k / n_fft);
        *p++ = (float)-std::sin(two_pi * k / n_fft);
    }
    for (int n = 0; n < n_fft; ++n) *p++ = (float)(0.5 - 0.5 * std::cos(two_pi * n / n_fft));
    return 0;
}

extern "C" int ldm_stft(const float* y, int32_t B, int64_t L, int32_t n_fft, int32_t hop, const float* tables, float* S,
                        float* mag, int32_t power, void* stream) {
    LDM_AUDIO_GEOMETRY("stft", n_fft, hop);
    LDM_REQUIRE(y && tables && (S || mag), "stft: null pointer");
    LDM_REQUIRE(B >= 1 && B <= 65535, "stft: B out of range");
    LDM_REQUIRE(L >= n_fft / 2 + 1, "stft: L too short for the reflect padding (needs L >= n_fft/2 + 1)");
    LDM_REQUIRE(L / hop < (1 << 30), "stft: L too long");
    LDM_REQUIRE(!mag || power == 1 || power == 2, "stft: power must be 1 or 2");
    StftOut o{reinterpret_cast<float2*>(S), mag, power, nullptr, nullptr, 0.f};
    return launch_stft(y, B, L, n_fft, (int)(1 + L / hop), tables, o, (hipStream_t)stream);
}

extern "C" int ldm_istft(const float* S, const float* mag, float* y, int32_t B, int32_t T, int64_t L, int32_t n_fft,
                         int32_t hop, const float* tables, void* stream) {
    LDM_AUDIO_GEOMETRY("istft", n_fft, hop);
    LDM_REQUIRE(S && y && tables, "istft: null pointer");
    LDM_REQUIRE(B >= 1 && B <= 65535 && T >= 1, "istft: B or T out of range");
    LDM_REQUIRE(L >= 1 && L <= (int64_t)(T + 1) * hop, "istft: L must lie within the frames' span, (T + 1) * hop");
    return launch_istft(S, mag, y, B, T, L, n_fft, tables, (hipStream_t)stream);
}

extern "C" int64_t ldm_griffinlim_workspace(int32_t B, int32_t n_fft, int32_t T) {
    if (B < 1 || T < 1 || !(n_fft == 512 || n_fft == 2048)) return 0;
    return 4 * (int64_t)B * (n_fft / 2 + 1) * T;   // r_prev and angles, complex
}

extern "C" int ldm_griffinlim(const float* mag, const float* init_angles, float* y, int32_t B, int32_t T, int64_t L,
                              int32_t n_fft, int32_t hop, int32_t n_iter, float momentum, const float* tables,
                              float* workspace, void* stream) {
    LDM_AUDIO_GEOMETRY("griffinlim", n_fft, hop);
    LDM_REQUIRE(mag && init_angles && y && tables && workspace, "griffinlim: null pointer");
    LDM_REQUIRE(B >= 1 && B <= 65535 && T >= 1, "griffinlim: B or T out of range");
    LDM_REQUIRE(L >= n_fft / 2 + 1 && 1 + L / hop == T, "griffinlim: L must give T frames (1 + L / hop == T) and be "
                                                       ">= n_fft/2 + 1");
    LDM_REQUIRE(n_iter >= 0 && momentum >= 0.f, "griffinlim: n_iter and momentum must be non-negative");
    return run_griffinlim(mag, init_angles, nullptr, nullptr, y, B, T, L, n_fft, n_iter, momentum, tables, workspace,
                          (hipStream_t)stream);
}

extern "C" int ldm_griffinlim_anchored(const float* mag, const float* init_angles, const float* anchor_phase,
                                       const float* anchor_w, float* y, int32_t B, int32_t T, int64_t L, int32_t n_fft,
                                       int32_t hop, int32_t n_iter, float momentum, const float* tables,
                                       float* workspace, void* stream) {
    LDM_AUDIO_GEOMETRY("griffinlim_anchored", n_fft, hop);
    LDM_REQUIRE(mag && init_angles && anchor_phase && anchor_w && y && tables && workspace,
                "griffinlim_anchored: null pointer");
    LDM_REQUIRE(B >= 1 && B <= 65535 && T >= 1, "griffinlim_anchored: B or T out of range");
    LDM_REQUIRE(L >= n_fft / 2 + 1 && 1 + L / hop == T, "griffinlim_anchored: L must give T frames (1 + L / hop == T) "
                                                       "and be >= n_fft/2 + 1");
    LDM_REQUIRE(n_iter >= 0 && momentum >= 0.f, "griffinlim_anchored: n_iter and momentum must be non-negative");
    return run_griffinlim(mag, init_angles, anchor_phase, anchor_w, y, B, T, L, n_fft, n_iter, momentum, tables,
                          workspace, (hipStream_t)stream);
}

extern "C" int ldm_mel_project(const float* P, const float* M, const int32_t* lohi, float* mel, int32_t B, int32_t F,
                               int32_t n_mels, int32_t T, void* stream) {
    LDM_REQUIRE(P && M && lohi && mel, "mel_project: null pointer");
    LDM_REQUIRE(B >= 1 && B <= 65535 && F >= 1 && n_mels >= 1 && T >= 1, "mel_project: bad shape");
    hipLaunchKernelGGL(mel_project_kernel, dim3((T + 63) / 64, (n_mels + 3) / 4, B), dim3(64, 4), 0, (hipStream_t)stream,
                       P, M, lohi, mel, F, n_mels, T);
    LDM_CHECK_LAUNCH("mel_project_kernel");
    return 0;
}

extern "C" int ldm_power_to_db(const float* x, float* out, int32_t B, int64_t n, float amin, float top_db,
                               float* workspace, void* stream) {
    LDM_REQUIRE(x && out && workspace, "power_to_db: null pointer");
    LDM_REQUIRE(B >= 1 && B <= 65535 && n >= 1 && amin > 0.f, "power_to_db: bad argument (B, n >= 1, amin > 0)");
    hipLaunchKernelGGL(db_ref_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, x, n, amin, workspace);
    LDM_CHECK_LAUNCH("db_ref_kernel");
    const unsigned gx = (unsigned)std::min<int64_t>((n + 255) / 256, 1024);
    hipLaunchKernelGGL(power_to_db_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, x, out, n, amin, top_db,
                       workspace);
    LDM_CHECK_LAUNCH("power_to_db_kernel");
    return 0;
}

extern "C" int ldm_db_to_power(const float* x, float* out, int64_t n, void* stream) {
    LDM_REQUIRE(x && out && n >= 0, "db_to_power: bad argument");
    if (n == 0) return 0;
    hipLaunchKernelGGL(db_to_power_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, x, out, n);
    LDM_CHECK_LAUNCH("db_to_power_kernel");
    return 0;
}

extern "C" int ldm_mel_invert(const float* mel, const float* M, const float* Mt, const float* Minv, const int32_t* lohi,
                              float inv_lambda, int32_t iters, int32_t take_sqrt, float* x, float* workspace, int32_t B,
                              int32_t F, int32_t n_mels, int32_t T, void* stream) {
    LDM_REQUIRE(mel && M && Mt && Minv && lohi && x && workspace, "mel_invert: null pointer");
    LDM_REQUIRE(B >= 1 && B <= 65535 && F >= 1 && n_mels >= 1 && T >= 1, "mel_invert: bad shape");
    LDM_REQUIRE(iters >= 0 && inv_lambda > 0.f, "mel_invert: iters >= 0 and 1/lambda > 0 required");
    hipStream_t st = (hipStream_t)stream;
    const dim3 gF((T + 63) / 64, (F + 63) / 64, B), gM((T + 63) / 64, (n_mels + 63) / 64, B);
    // x0 = max(M^+ mel, 0)
    hipLaunchKernelGGL(gemm_kernel<0>, gF, dim3(256), 0, st, Minv, mel, x, (const float*)nullptr, (const int32_t*)nullptr,
                       F, n_mels, T, 0.f);
    LDM_CHECK_LAUNCH("gemm_kernel<0>");
    for (int it = 0; it < iters; ++it) {
        // r = M x - mel;  x = max(x - M^T r / lambda, 0)
        hipLaunchKernelGGL(gemm_kernel<1>, gM, dim3(256), 0, st, M, (const float*)x, workspace, mel, lohi, n_mels, F, T,
                           0.f);
        LDM_CHECK_LAUNCH("gemm_kernel<1>");
        hipLaunchKernelGGL(gemm_kernel<2>, gF, dim3(256), 0, st, Mt, (const float*)workspace, x, (const float*)nullptr,
                           (const int32_t*)nullptr, F, n_mels, T, inv_lambda);
        LDM_CHECK_LAUNCH("gemm_kernel<2>");
    }
    if (take_sqrt) {
        const int64_t n = (int64_t)B * F * T;
        hipLaunchKernelGGL(sqrt_kernel, dim3(grid_for(n)), dim3(256), 0, st, x, n);
        LDM_CHECK_LAUNCH("sqrt_kernel");
    }
    return 0;
}
