// Whole-recording front and back end of the model's windows.  A recording's mel power
// P [n_mels, T_total] is cut into N windows of `frames` frames that start every stride = frames - overlap frames
// (frames at or beyond T_total hold zero power); each window becomes the model's [0,1] input referred to its own
// maximum, and the decoded windows are put back into one mel power map with a linear crossfade in dB over each
// overlap.  overlap <= frames / 2, so at most two windows cover a frame.
//
// Both passes are elementwise and byte-bound: one lane per element, frames (t) fastest in every load and store,
// 64-bit offsets, no atomics, no unfolded copy of P.  The arithmetic is mel_db.h's, shared with the kernels
// whose composition ldm_mel_windows equals bitwise (power_to_db, mel_quantize, u8_to_unit).
#include "common.h"
#include "mel_db.h"

#include <algorithm>

namespace ldm {
namespace {

constexpr int kRefThreads = 1024;

// ref[n] = 10 log10(max(amin, max of window n)).  One block per window; max is exact in any order.
__global__ __launch_bounds__(kRefThreads) void mel_window_ref_kernel(const float* __restrict__ P, int n_mels,
                                                                     int64_t T, int frames, FastDiv fd_frames, int stride,
                                                                     float amin, float* __restrict__ ref) {
    __shared__ float s[kRefThreads];
    const int64_t t0 = (int64_t)blockIdx.x * stride;
    const int per = n_mels * frames;   // < 2^30 (checked by the entry)
    auto at = [&](int i) {
        const int mel = fd_frames.div(i), j = i - mel * frames;
        const int64_t t = t0 + j;
        return t < T ? P[(int64_t)mel * T + t] : 0.f;
    };
    // 18 blocks cover a 3-minute recording, so a lane's loads are what hides the latency: 8 in flight at a time
    constexpr int kU = 8;
    float m = -INFINITY;
    int i = threadIdx.x;
    for (; i + (kU - 1) * kRefThreads < per; i += kU * kRefThreads) {
        float v[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) v[u] = at(i + u * kRefThreads);
#pragma unroll
        for (int u = 0; u < kU; ++u) m = fmaxf(m, v[u]);
    }
    for (; i < per; i += kRefThreads) m = fmaxf(m, at(i));
    s[threadIdx.x] = m;
    __syncthreads();
    for (int w = kRefThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] = fmaxf(s[threadIdx.x], s[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) ref[blockIdx.x] = db_ref(s[0], amin);
}

// x[n, 0, mel, j] = unit(quant(db(P[mel, n stride + j]) - ref[n])).  grid (blocks, N), grid-stride over a window.
__global__ __launch_bounds__(256) void mel_windows_kernel(const float* __restrict__ P, int n_mels, int64_t T, int frames,
                                                          FastDiv fd_frames, int stride, float amin, float top_db,
                                                          float max_db, float scale, const float* __restrict__ ref,
                                                          float* __restrict__ x) {
    const int n = blockIdx.y;
    const float r = ref[n];
    const int64_t t0 = (int64_t)n * stride;
    const int per = n_mels * frames;
    float* xn = x + (int64_t)n * per;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < per; i += gridDim.x * 256) {
        const int mel = fd_frames.div(i), j = i - mel * frames;
        const int64_t t = t0 + j;
        const float p = t < T ? P[(int64_t)mel * T + t] : 0.f;
        xn[i] = unit1(quant1(power_db1(p, amin, top_db, r), max_db, scale));
    }
}

// dB of a decoded pixel: clamp(y, 0, 1) * max_db - max_db + ref
__device__ __forceinline__ float window_db(float y, float max_db, float ref) {
#pragma clang fp contract(off)
    const float c = fminf(fmaxf(y, 0.f), 1.f);
    const float v = c * max_db;
    return (v - max_db) + ref;
}

// One lane per output (mel, t), t fastest.  grid (ceil(T / 256), n_mels).
__global__ __launch_bounds__(256) void mel_stitch_kernel(const float* __restrict__ y, const float* __restrict__ ref, int N,
                                                         int n_mels, int frames, int stride, FastDiv fd_stride, int overlap,
                                                         int T, float max_db, float* __restrict__ power,
                                                         float* __restrict__ db_out) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * 256 + threadIdx.x, mel = blockIdx.y;
    if (t >= T) return;
    const int n1 = min(N - 1, fd_stride.div(t)), j1 = t - n1 * stride;   // j1 < frames: T <= (N - 1) stride + frames
    const int64_t row = (int64_t)n_mels * frames;
    const float* y1 = y + (int64_t)n1 * row + (int64_t)mel * frames;
    float db = window_db(y1[j1], max_db, ref[n1]);
    if (n1 >= 1 && j1 < overlap) {   // the tail of window n1 - 1 fades out as window n1 fades in
        const float d0 = window_db(y1[j1 + stride - row], max_db, ref[n1 - 1]);
        const float span = (float)(overlap + 1);
        const float w0 = (float)(overlap - j1) / span, w1 = (float)(j1 + 1) / span;
        db = w0 * d0 + w1 * db;
    }
    const int64_t at = (int64_t)mel * T + t;
    power[at] = db_power1(db);
    if (db_out) db_out[at] = db;
}

// N of the window plan, or 0 for a bad plan
int64_t plan_windows(int64_t T, int frames, int overlap) {
    if (T < 1 || frames < 64 || frames % 64 != 0 || overlap < 0 || overlap > frames / 2) return 0;
    const int64_t stride = frames - overlap, n = (T - overlap + stride - 1) / stride;
    return n < 1 ? 1 : n;
}

}  // namespace
}  // namespace ldm

using namespace ldm;

extern "C" int64_t ldm_mel_window_count(int64_t T_total, int32_t frames, int32_t overlap) {
    return plan_windows(T_total, frames, overlap);
}

extern "C" int ldm_mel_windows(const float* P, int32_t n_mels, int64_t T_total, int32_t frames, int32_t overlap,
                               float amin, float top_db, float max_db, float* x, float* ref_db, void* stream) {
    LDM_REQUIRE(P && x && ref_db, "mel_windows: null pointer");
    const int64_t N = plan_windows(T_total, frames, overlap);
    LDM_REQUIRE(N >= 1, "mel_windows: bad plan (T_total >= 1, frames a multiple of 64, 0 <= overlap <= frames / 2)");
    LDM_REQUIRE(N <= 65535, "mel_windows: more than 65535 windows");
    LDM_REQUIRE(n_mels >= 1 && (int64_t)n_mels * frames < (1LL << 30), "mel_windows: n_mels * frames out of range");
    LDM_REQUIRE(amin > 0.f && max_db > 0.f, "mel_windows: amin and max_db must be positive");
    const int stride = frames - overlap, per = n_mels * frames;
    hipLaunchKernelGGL(mel_window_ref_kernel, dim3((unsigned)N), dim3(kRefThreads), 0, (hipStream_t)stream, P, n_mels,
                       T_total, frames, FastDiv::make(frames), stride, amin, ref_db);
    LDM_CHECK_LAUNCH("mel_window_ref_kernel");
    const unsigned gx = (unsigned)std::min<int64_t>(((int64_t)per + 255) / 256, 1024);
    hipLaunchKernelGGL(mel_windows_kernel, dim3(gx, (unsigned)N), dim3(256), 0, (hipStream_t)stream, P, n_mels, T_total,
                       frames, FastDiv::make(frames), stride, amin, top_db, max_db, (float)(255.0 / (double)max_db),
                       (const float*)ref_db, x);
    LDM_CHECK_LAUNCH("mel_windows_kernel");
    return 0;
}

extern "C" int ldm_mel_stitch(const float* y, const float* ref_db, int32_t N, int32_t n_mels, int32_t frames,
                              int32_t overlap, int64_t T_total, float max_db, float* power, float* db, void* stream) {
    LDM_REQUIRE(y && ref_db && power, "mel_stitch: null pointer");
    const int64_t want = plan_windows(T_total, frames, overlap);
    LDM_REQUIRE(want >= 1, "mel_stitch: bad plan (T_total >= 1, frames a multiple of 64, 0 <= overlap <= frames / 2)");
    LDM_REQUIRE(N == want, "mel_stitch: N is not the window count of (T_total, frames, overlap)");
    LDM_REQUIRE(T_total <= (1LL << 31) - 512, "mel_stitch: T_total out of range");
    LDM_REQUIRE(n_mels >= 1 && n_mels <= 65535 && (int64_t)n_mels * frames < (1LL << 30),
                "mel_stitch: n_mels out of range");
    LDM_REQUIRE(max_db > 0.f, "mel_stitch: max_db must be positive");
    const int T = (int)T_total;
    hipLaunchKernelGGL(mel_stitch_kernel, dim3((unsigned)((T + 255) / 256), (unsigned)n_mels), dim3(256), 0,
                       (hipStream_t)stream, y, ref_db, N, n_mels, frames, frames - overlap,
                       FastDiv::make(frames - overlap), overlap, T, max_db, power, db);
    LDM_CHECK_LAUNCH("mel_stitch_kernel");
    return 0;
}
