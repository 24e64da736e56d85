// The content-anchored vocoder's streaming kernels: the transfer read as an edit of the content's own
// STFT.  The model's mel-domain gain G = (Mo + eps) / (Mc + eps) is carried to the linear bins through the filterbank
// normalised per bin, Wn[m, f] = M[m, f] / sum_m' M[m', f], and applied to the content's power:
//   g = clamp(sum_m Wn[m, f] G[m, t], 0, max_gain)      (1 for a bin no filter covers)
//   Pm = g |C|^2,   A = sqrt(Pm + R),   P0 = C / |C|  ((1, 0) where |C| < kTiny),
//   a = clamp(1 - |10 log10((A^2 + eps) / (|C|^2 + eps))| / anchor_db, 0, 1)    (0 when anchor_db <= 0)
// The sum runs as 1 + sum_m Wn (G - 1): the same number (sum_m Wn = 1), and exactly 1 where the mel did not change, so
// an untouched bin keeps |C| and gets a = 1 bitwise.
//
// One lane per (f, t), t fastest, the layout of every [B, F, T] tensor here: C, R and the three outputs move in
// coalesced 256- / 512-byte runs per wave, C is read once, g lives in a register.  A wave shares its bin, so the
// filter range [m_lo, m_hi) (at most a few filters of a triangular bank; the host's table, the transpose of the
// mel projection's lohi) and the weights Wn[m, f] are uniform loads, and the mel rows it reads are shared with the
// neighbouring bins' waves (n_mels / F of the traffic, from L2).
#include "common.h"

#include <cmath>

namespace ldm {
namespace {

constexpr float kTiny = 1.17549435e-38f;   // smallest normal fp32 (as audio.hip)

// block (64, 4), grid (ceil(T / 64), ceil(F / 4), B).  TARGET false: out = Pm.  TARGET true: out = A, P0, aw.
template <bool TARGET>
__global__ __launch_bounds__(256) void mel_gain_kernel(const float2* __restrict__ C, const float* __restrict__ Mo,
                                                       const float* __restrict__ Mc, const float* __restrict__ Wn,
                                                       const int32_t* __restrict__ mlohi, const float* __restrict__ eps,
                                                       float max_gain, float anchor_db, const float* __restrict__ R,
                                                       float* __restrict__ out, float2* __restrict__ P0,
                                                       float* __restrict__ aw, int F, int n_mels, int T) {
    const int t = blockIdx.x * 64 + threadIdx.x, f = blockIdx.y * 4 + threadIdx.y, b = blockIdx.z;
    if (f >= F || t >= T) return;
    const float e = eps[b];
    const int lo = max(mlohi[2 * f], 0), hi = min(mlohi[2 * f + 1], n_mels);
    const float* mo = Mo + (int64_t)b * n_mels * T + t;
    const float* mc = Mc + (int64_t)b * n_mels * T + t;
    float g = 1.f;
    for (int m = lo; m < hi; ++m) {
        const float G = (mo[(int64_t)m * T] + e) / (mc[(int64_t)m * T] + e);
        g = fmaf(Wn[(int64_t)m * F + f], G - 1.f, g);
    }
    g = fminf(fmaxf(g, 0.f), max_gain);
    const int64_t at = ((int64_t)b * F + f) * T + t;
    const float2 c = C[at];
    const float p2 = c.x * c.x + c.y * c.y;
    const float pm = g * p2;
    if constexpr (!TARGET) {
        out[at] = pm;
    } else {
        const float a2 = R ? pm + R[at] : pm;
        out[at] = sqrtf(a2);
        // |C| below 1e-15 squares into the denormals: take the modulus of 2^64 C there
        float sx = c.x, sy = c.y, lim = kTiny;
        if (p2 < 1e-30f) sx *= 0x1p+64f, sy *= 0x1p+64f, lim = kTiny * 0x1p+64f;
        const float mod = sqrtf(sx * sx + sy * sy);
        P0[at] = mod < lim ? make_float2(1.f, 0.f) : make_float2(sx / mod, sy / mod);
        float w = 0.f;
        if (anchor_db > 0.f) {
            const float d = 10.f * log10f((a2 + e) / (p2 + e));
            w = fminf(fmaxf(1.f - fabsf(d) / anchor_db, 0.f), 1.f);
        }
        aw[at] = w;
    }
}

}  // namespace
}  // namespace ldm

using namespace ldm;

#define LDM_GAIN_SHAPE(what)                                                                                    \
    LDM_REQUIRE(B >= 1 && B <= 65535 && F >= 1 && F <= 4 * 65535 && n_mels >= 1 && T >= 1, what ": bad shape"); \
    LDM_REQUIRE(std::isfinite(max_gain) && max_gain >= 0.f, what ": max_gain must be finite and non-negative")

extern "C" int ldm_mel_gain_power(const float* C, const float* mel_out, const float* mel_content, const float* Wn,
                                  const int32_t* mlohi, const float* eps, float max_gain, float* Pm, int32_t B, int32_t F,
                                  int32_t n_mels, int32_t T, void* stream) {
    LDM_REQUIRE(C && mel_out && mel_content && Wn && mlohi && eps && Pm, "mel_gain_power: null pointer");
    LDM_GAIN_SHAPE("mel_gain_power");
    hipLaunchKernelGGL(mel_gain_kernel<false>, dim3((T + 63) / 64, (F + 3) / 4, B), dim3(64, 4), 0, (hipStream_t)stream,
                       reinterpret_cast<const float2*>(C), mel_out, mel_content, Wn, mlohi, eps, max_gain, 0.f,
                       (const float*)nullptr, Pm, (float2*)nullptr, (float*)nullptr, F, n_mels, T);
    LDM_CHECK_LAUNCH("mel_gain_kernel<false>");
    return 0;
}

extern "C" int ldm_mel_gain_target(const float* C, const float* mel_out, const float* mel_content, const float* Wn,
                                   const int32_t* mlohi, const float* eps, float max_gain, float anchor_db,
                                   const float* residual, float* mag, float* phase0, float* anchor, int32_t B, int32_t F,
                                   int32_t n_mels, int32_t T, void* stream) {
    LDM_REQUIRE(C && mel_out && mel_content && Wn && mlohi && eps && mag && phase0 && anchor,
                "mel_gain_target: null pointer");
    LDM_GAIN_SHAPE("mel_gain_target");
    LDM_REQUIRE(std::isfinite(anchor_db), "mel_gain_target: anchor_db must be finite");
    hipLaunchKernelGGL(mel_gain_kernel<true>, dim3((T + 63) / 64, (F + 3) / 4, B), dim3(64, 4), 0, (hipStream_t)stream,
                       reinterpret_cast<const float2*>(C), mel_out, mel_content, Wn, mlohi, eps, max_gain, anchor_db,
                       residual, mag, reinterpret_cast<float2*>(phase0), anchor, F, n_mels, T);
    LDM_CHECK_LAUNCH("mel_gain_kernel<true>");
    return 0;
}
