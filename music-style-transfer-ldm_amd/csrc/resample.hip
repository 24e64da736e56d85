// The two steps in front of the audio transforms: a rational polyphase resampler and librosa's
// silence trim.  All fp32, batched, on the caller's stream, no atomics: every output is one sum in a fixed order.
//
// Resampler.  y[n] = sum_{j=-W..W} x[i0 + j] * taps[p][j + W],  i0 = floor(n down / up),  p = (n down) mod up,
// x zero outside [0, L).  taps [up, 2W+1] is the caller's table (ldm_amd.audio.resample_taps: Kaiser-windowed sinc).
//
// A workgroup owns kR * U consecutive outputs, U = m * up a multiple of `up`, starting at a multiple of U.  Such a
// start has phase 0 and an exact input position (n0 / up) * down, so inside the tile every index is a small 32-bit
// offset from one 64-bit base: no 64-bit division in the kernel and no overflow at n * down > 2^32.  Lane u < U
// computes the kR outputs n0 + u + r U: they share the phase (u down) mod up, so one tap load feeds kR FMAs, and
// their inputs lie r * m * down apart.  Lanes u, u + 1 store neighbouring outputs (coalesced).
//
// LDS: the tile's input span floor((kR U - 1) down / up) + 2W + 1 floats (<= kSpanCap = 32 KB), decoded once (the
// int16 form mixes its channels here), and the tap table when it has <= kTapsCap floats (32 KB: every integer
// ratio and the small `up`s); a larger table (147 x 149 for 48000 -> 22050, 87 KB) is read from global memory,
// where it stays L2-resident and each lane walks its own row.  The host picks m for the fullest 256-lane passes
// within the span cap.  Banks (ds_read_b32: 32 banks per 32-lane half): neighbouring lanes read x at a stride of
// down / up floats, i.e. about max(1, down / up)-way conflicts on the input reads (2-way for 2:1), and the tap read
// is a broadcast for up == 1 and one row of odd pitch per lane otherwise.
//
// Trim.  frame_ms_kernel: one wave per frame, mean square of the centred zero-padded frame, lane partial sums in a
// fixed stride then a butterfly.  trim_bounds_kernel: one workgroup per item, the item maximum, then the first and
// last frame above the threshold, as an int64 pair.
#include "common.h"

#include <algorithm>
#include <cmath>

namespace ldm {
namespace {

constexpr int kR = 4;            // outputs per lane, one phase
constexpr int kThreads = 256;
constexpr int kSpanCap = 8192;   // floats of input per workgroup
constexpr int kTapsCap = 8192;   // largest tap table kept in LDS (floats)
constexpr int kMaxU = 1024;

struct F32In {
    const float* x;   // [B, L]
    __device__ __forceinline__ float at(int b, int64_t L, int64_t i) const { return x[(int64_t)b * L + i]; }
};

struct Pcm16In {
    const int16_t* x;   // [L, ch] interleaved
    int ch;
    // the mean over channels of s / 32768, as numpy's float32 mean of the decoded frame (exact for ch <= 2)
    __device__ __forceinline__ float at(int, int64_t, int64_t i) const {
        const int16_t* f = x + i * ch;
        float s = 0.f;
        for (int c = 0; c < ch; ++c) s += (float)f[c] * (1.0f / 32768.0f);
        return s / (float)ch;
    }
};

// grid (ceil(n_out / (kR U)), B), dynamic LDS (span + (TAPS_LDS ? up (2W+1) : 0)) floats
template <typename In, bool TAPS_LDS>
__global__ __launch_bounds__(kThreads) void resample_kernel(In in, int64_t L, const float* __restrict__ taps, int up,
                                                            int down, int W, int U, int span, float* __restrict__ y,
                                                            int64_t n_out) {
    extern __shared__ float smem[];
    float* sx = smem;
    float* st = smem + span;
    const int K = 2 * W + 1;
    const int b = blockIdx.y;
    const int step = (U / up) * down;                       // input distance between a lane's outputs
    const int64_t n0 = (int64_t)blockIdx.x * kR * U;
    const int64_t s0 = (int64_t)blockIdx.x * kR * step - W;   // = (n0 / up) * down - W
    for (int i = threadIdx.x; i < span; i += kThreads) {
        const int64_t g = s0 + i;
        sx[i] = (g >= 0 && g < L) ? in.at(b, L, g) : 0.f;
    }
    if (TAPS_LDS)
        for (int i = threadIdx.x; i < up * K; i += kThreads) st[i] = taps[i];
    __syncthreads();
    const float* tp = TAPS_LDS ? st : taps;
    for (int u = threadIdx.x; u < U; u += kThreads) {
        const int q = u * down, off = q / up, p = q - off * up;
        const float* h = tp + p * K;
        const float* xs = sx + off;   // off + (kR - 1) step + 2W <= span - 1
        float acc[kR] = {};
        for (int j = 0; j < K; ++j) {
            const float c = h[j];
#pragma unroll
            for (int r = 0; r < kR; ++r) acc[r] = fmaf(xs[r * step + j], c, acc[r]);
        }
#pragma unroll
        for (int r = 0; r < kR; ++r) {
            const int64_t n = n0 + u + (int64_t)r * U;
            if (n < n_out) y[(int64_t)b * n_out + n] = acc[r];
        }
    }
}

int64_t span_of(int U, int up, int down, int W) { return ((int64_t)kR * U - 1) * down / up + 2 * W + 1; }

template <typename In>
int launch_resample(In in, int B, int64_t L, const float* taps, int up, int down, int W, float* y, hipStream_t st) {
    const int64_t n_out = (L * up + down - 1) / down;
    // U = m up <= kMaxU whose span fits: the fullest 256-lane passes, the larger tile on a tie
    int bestU = 0;
    double best = 0.0;
    for (int U = up; U <= kMaxU; U += up) {
        if (span_of(U, up, down, W) > kSpanCap) break;
        const double fill = (double)U / (double)((U + kThreads - 1) / kThreads * kThreads);
        if (fill >= best) best = fill, bestU = U;
    }
    LDM_REQUIRE(bestU > 0, "resample: this ratio needs more than the 32 KB input tile (up <= 1024 and about "
                           "4 down + 2 W <= 8192 are supported)");
    const int U = bestU, span = (int)span_of(U, up, down, W);
    const int64_t blocks = (n_out + (int64_t)kR * U - 1) / ((int64_t)kR * U);
    LDM_REQUIRE(blocks <= 0x7fffffff, "resample: L too long");
    const bool lds_taps = (int64_t)up * (2 * W + 1) <= kTapsCap;
    const size_t lds = sizeof(float) * (size_t)(span + (lds_taps ? up * (2 * W + 1) : 0));
    const dim3 grid((unsigned)blocks, B);
    if (lds_taps)
        hipLaunchKernelGGL((resample_kernel<In, true>), grid, dim3(kThreads), lds, st, in, L, taps, up, down, W, U, span,
                           y, n_out);
    else
        hipLaunchKernelGGL((resample_kernel<In, false>), grid, dim3(kThreads), lds, st, in, L, taps, up, down, W, U, span,
                           y, n_out);
    LDM_CHECK_LAUNCH("resample_kernel");
    return 0;
}

// grid (ceil(T / 4), B), one wave per frame.  ms [B, T]
__global__ __launch_bounds__(kThreads) void frame_ms_kernel(const float* __restrict__ y, int64_t L, int T, int frame,
                                                            int hop, float* __restrict__ ms) {
    const int t = blockIdx.x * (kThreads / 64) + threadIdx.x / 64, lane = threadIdx.x % 64, b = blockIdx.y;
    if (t >= T) return;
    const float* yb = y + (int64_t)b * L;
    const int64_t s = (int64_t)t * hop - frame / 2;
    float acc = 0.f;
    for (int i = lane; i < frame; i += 64) {
        const int64_t g = s + i;
        const float v = (g >= 0 && g < L) ? yb[g] : 0.f;
        acc = fmaf(v, v, acc);
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) ms[(int64_t)b * T + t] = acc / (float)frame;
}

// grid (B).  bounds [B][2] = {hop * first, min(L, hop * (last + 1))} over the frames with
// max(ms, floor) > max(max ms, floor) * thr; {0, 0} when there is none, or when max ms <= floor.
__global__ __launch_bounds__(kThreads) void trim_bounds_kernel(const float* __restrict__ ms, int T, int64_t L, int hop,
                                                               float thr, float floor_, int64_t* __restrict__ bounds) {
    __shared__ float s_max[kThreads];
    __shared__ int s_first[kThreads], s_last[kThreads];
    const float* m = ms + (int64_t)blockIdx.x * T;
    const int tid = threadIdx.x;
    float mx = 0.f;
    for (int t = tid; t < T; t += kThreads) mx = fmaxf(mx, m[t]);
    s_max[tid] = mx;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if (tid < w) s_max[tid] = fmaxf(s_max[tid], s_max[tid + w]);
        __syncthreads();
    }
    mx = s_max[0];
    const float cut = fmaxf(mx, floor_) * thr;
    int first = T, last = -1;
    if (mx > floor_)
        for (int t = tid; t < T; t += kThreads)
            if (fmaxf(m[t], floor_) > cut) first = min(first, t), last = max(last, t);
    s_first[tid] = first;
    s_last[tid] = last;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if (tid < w) {
            s_first[tid] = min(s_first[tid], s_first[tid + w]);
            s_last[tid] = max(s_last[tid], s_last[tid + w]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        const bool any = s_last[0] >= 0;
        bounds[2 * blockIdx.x] = any ? (int64_t)hop * s_first[0] : 0;
        bounds[2 * blockIdx.x + 1] = any ? std::min<int64_t>(L, (int64_t)hop * (s_last[0] + 1)) : 0;
    }
}

bool ratio_ok(int up, int down, int W) {
    return up >= 1 && down >= 1 && up <= kMaxU && down <= (1 << 20) && W >= 0 && W <= kSpanCap;
}

}  // namespace
}  // namespace ldm

using namespace ldm;

extern "C" int64_t ldm_resample_out_len(int64_t L, int32_t up, int32_t down) {
    if (L < 0 || up < 1 || down < 1 || L > ((int64_t)1 << 40) || up > (1 << 20)) return 0;
    return (L * up + down - 1) / down;
}

extern "C" int ldm_resample_f32(const float* x, int32_t B, int64_t L, const float* taps, int32_t up, int32_t down,
                                int32_t W, float* y, void* stream) {
    LDM_REQUIRE(x && taps && y, "resample_f32: null pointer");
    LDM_REQUIRE(B >= 1 && B <= 65535, "resample_f32: B out of range");
    LDM_REQUIRE(L >= 1 && L <= ((int64_t)1 << 40), "resample_f32: L out of range");
    LDM_REQUIRE(ratio_ok(up, down, W), "resample_f32: up, down or W out of range");
    return launch_resample(F32In{x}, B, L, taps, up, down, W, y, (hipStream_t)stream);
}

extern "C" int ldm_resample_pcm16(const int16_t* pcm, int64_t L, int32_t channels, const float* taps, int32_t up,
                                  int32_t down, int32_t W, float* y, void* stream) {
    LDM_REQUIRE(pcm && taps && y, "resample_pcm16: null pointer");
    LDM_REQUIRE(channels >= 1 && channels <= 64, "resample_pcm16: 1 to 64 channels");
    LDM_REQUIRE(L >= 1 && L <= ((int64_t)1 << 40), "resample_pcm16: L out of range");
    LDM_REQUIRE(ratio_ok(up, down, W), "resample_pcm16: up, down or W out of range");
    return launch_resample(Pcm16In{pcm, channels}, 1, L, taps, up, down, W, y, (hipStream_t)stream);
}

extern "C" int64_t ldm_trim_workspace_floats(int32_t B, int64_t L, int32_t hop) {
    if (B < 1 || L < 1 || hop < 1) return 0;
    return (int64_t)B * (1 + L / hop);
}

extern "C" int ldm_trim_bounds(const float* y, int32_t B, int64_t L, int32_t frame_length, int32_t hop, float top_db,
                               float* workspace, int64_t* bounds, void* stream) {
    LDM_REQUIRE(y && workspace && bounds, "trim_bounds: null pointer");
    LDM_REQUIRE(B >= 1 && B <= 65535 && L >= 1, "trim_bounds: B or L out of range");
    LDM_REQUIRE(frame_length >= 1 && hop >= 1 && L / hop < (1 << 30), "trim_bounds: bad frame_length or hop");
    const int T = (int)(1 + L / hop);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(frame_ms_kernel, dim3((T + 3) / 4, B), dim3(kThreads), 0, st, y, L, T, frame_length, hop,
                       workspace);
    LDM_CHECK_LAUNCH("frame_ms_kernel");
    const float thr = (float)std::pow(10.0, -(double)top_db / 10.0);
    hipLaunchKernelGGL(trim_bounds_kernel, dim3(B), dim3(kThreads), 0, st, (const float*)workspace, T, L, hop, thr,
                       1e-10f, bounds);
    LDM_CHECK_LAUNCH("trim_bounds_kernel");
    return 0;
}
