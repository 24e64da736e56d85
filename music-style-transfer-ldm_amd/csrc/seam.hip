// Joint sampling of overlapping windows: the seam fuse of the reverse loop's state.
//
// The batch rows of x [B, C, H, W] are neighbouring windows of one recording: row b's last `ov` latent columns and
// row b + 1's first `ov` cover the same frames.  One fuse replaces both copies by one weighted average, per element
// (seam_blend below), so that after it x[b, :, :, W-ov+j] == x[b+1, :, :, j] bitwise.  ov <= W / 2 keeps a row's left
// and right seam columns disjoint: every element belongs to at most one seam, each seam element pair is read and
// written by exactly one lane, and the fuse is safe in place with no ordering between lanes.
//
// One kernel, two layouts: NHWC (the step kernels' state ws.xs; one lane per four channels, 128-bit accesses along C)
// and NCHW (conv.hip's loops and the public entry; one lane per element, the seam column fastest).  One launch covers
// every seam of `groups` independent stacks of B rows (the guided loop's target and base halves: no seam between row
// B - 1 and row B).  Byte-bound and tiny (2 ov / W of the state): no LDS, no atomics, no cross-block hand-off.
#include "common.h"

namespace ldm {
namespace {

// One seam element: a from the earlier window's tail, q from the later window's head, wj = (j + 1) / (ov + 1) the
// later window's weight (its weight in the crossfade of stitch_windows, at latent granularity).  fp32, one rounding per
// operation, as keep_blend.
__device__ __forceinline__ float seam_blend(float a, float q, float wj) {
#pragma clang fp contract(off)
    const float d = q - a;
    const float p = wj * d;
    return a + p;
}

// n lanes.  NHWC: lane = (((g (B-1) + b) H + h) ov + j) C/4 + c4;  NCHW: lane = (((g (B-1) + b) C + c) H + h) ov + j.
template <bool NHWC>
__global__ __launch_bounds__(256) void seam_fuse_kernel(float* __restrict__ x, int B, int C, int H, int W, int ov,
                                                        int64_t n) {
#pragma clang fp contract(off)
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float span = (float)(ov + 1);
    if constexpr (NHWC) {
        const int C4 = C >> 2;
        const int c4 = (int)(i % C4);
        i /= C4;
        const int j = (int)(i % ov);
        i /= ov;
        const int h = (int)(i % H);
        i /= H;
        const int64_t b = i % (B - 1), g = i / (B - 1);
        const int64_t row = g * B + b;   // the earlier window; row + 1 <= groups * B - 1
        const int64_t plane = (int64_t)H * W;
        floatx4* pa = reinterpret_cast<floatx4*>(x + ((row * plane + (int64_t)h * W + (W - ov + j)) * C + 4 * c4));
        floatx4* pq = reinterpret_cast<floatx4*>(x + (((row + 1) * plane + (int64_t)h * W + j) * C + 4 * c4));
        const floatx4 a = *pa, q = *pq;
        const float wj = (float)(j + 1) / span;
        floatx4 m;
        m.x = seam_blend(a.x, q.x, wj);
        m.y = seam_blend(a.y, q.y, wj);
        m.z = seam_blend(a.z, q.z, wj);
        m.w = seam_blend(a.w, q.w, wj);
        *pa = m;
        *pq = m;
    } else {
        const int j = (int)(i % ov);
        i /= ov;
        const int h = (int)(i % H);
        i /= H;
        const int c = (int)(i % C);
        i /= C;
        const int64_t b = i % (B - 1), g = i / (B - 1);
        const int64_t row = g * B + b;
        const int64_t plane = (int64_t)H * W;
        float* pa = x + ((row * C + c) * plane + (int64_t)h * W + (W - ov + j));
        float* pq = x + (((row + 1) * C + c) * plane + (int64_t)h * W + j);
        const float m = seam_blend(*pa, *pq, (float)(j + 1) / span);
        *pa = m;
        *pq = m;
    }
}

}  // namespace

// x: `groups` stacks of B rows [C, H, W] (NCHW) or [H, W, C] (nhwc; C % 4 == 0, x 16-byte aligned).  B == 1 or
// ov == 0: nothing to launch.
int seam_fuse(float* x, int groups, int B, int C, int H, int W, int ov, bool nhwc, hipStream_t st) {
    LDM_REQUIRE(x && groups >= 1 && B >= 1 && C >= 1 && H >= 1 && W >= 2, "seam_fuse: bad argument");
    LDM_REQUIRE(ov >= 0 && ov <= W / 2, "seam_fuse: seam_cols must lie in [0, W / 2]");
    if (B == 1 || ov == 0) return 0;
    const int64_t pairs = (int64_t)groups * (B - 1) * C * H * ov;
    if (nhwc) {
        LDM_REQUIRE(C % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0,
                    "seam_fuse: the NHWC form needs C % 4 == 0 and a 16-byte aligned state");
        const int64_t n = pairs / 4;
        hipLaunchKernelGGL(seam_fuse_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, B, C, H, W, ov, n);
    } else {
        hipLaunchKernelGGL(seam_fuse_kernel<false>, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st, x, B, C, H, W,
                           ov, pairs);
    }
    LDM_CHECK_LAUNCH("seam_fuse_kernel");
    return 0;
}

}  // namespace ldm

using namespace ldm;

extern "C" int ldm_seam_fuse(float* x, int32_t B, int32_t C, int32_t H, int32_t W, int32_t seam_cols, void* stream) {
    LDM_REQUIRE(x && B >= 1 && C >= 1 && H >= 1 && W >= 2, "seam_fuse: bad argument");
    LDM_REQUIRE(seam_cols >= 1 && seam_cols <= W / 2, "seam_fuse: seam_cols must lie in [1, W / 2]");
    LDM_REQUIRE((int64_t)B * C * H * W < (1LL << 40), "seam_fuse: tensor out of range");
    return seam_fuse(x, 1, B, C, H, W, seam_cols, false, (hipStream_t)stream);
}
