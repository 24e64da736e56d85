// Optimizer kernels of the LDM train step: multi-tensor Adam / AdamW (torch.optim.Adam, train.py:156) with
// GradScaler unscale / inf check / skip / scale update (train.py:157,189-201), and, off by default, gradient-norm
// clipping and an EMA of the weights inside the same launches.
// Every kernel walks a chunk map: block i works on chunk_len elements of tensor chunk_tensor[i] from chunk_start[i].
// Every reduction has a fixed partition and order: results are bitwise reproducible run to run.
#include <cmath>

#include "common.h"

#pragma clang fp contract(off)

namespace ldm {

// The chunk of blockIdx.x: its slot, the slot's index, and the element range [s0, e0).  Under LDM_DEBUG_BOUNDS
// (common.h) a chunk whose map entry cannot be trusted is printed and refused instead of dereferenced.
struct Chunk {
    ldm_tensor_slot sl;
    int32_t ti;
    int64_t s0, e0;
};
__device__ __forceinline__ bool chunk_open(const char* kname, const ldm_tensor_slot* __restrict__ slots,
                                           const int32_t* __restrict__ chunk_tensor,
                                           const int64_t* __restrict__ chunk_start, int chunk_len, Chunk& c) {
    c.ti = chunk_tensor[blockIdx.x];
#if LDM_DEBUG_BOUNDS
    const bool bad_ix = c.ti < 0 || c.ti >= (int32_t)gridDim.x || chunk_start[blockIdx.x] < 0;
    if (bad_ix || slots[c.ti].grad == nullptr) {
        if (threadIdx.x == 0) printf("%s: chunk %u: bad slot index %d / start %ld\n", kname, blockIdx.x, c.ti, (long)chunk_start[blockIdx.x]);
        return false;
    }
#endif
    c.sl = slots[c.ti];   // before chunk_start: read the other way round, the slot loads wait for both (+1 us per step)
    c.s0 = chunk_start[blockIdx.x];
    c.e0 = min(c.s0 + (int64_t)chunk_len, c.sl.numel);
    return true;
}

// A chunk's elements, float4 at a time where every pointer of the slot is 16-byte aligned (the chunk
// start is a multiple of 4 elements), the ragged tail one at a time; f(i, W) handles elements i..i+W-1.
template <class F4, class F1>
__device__ __forceinline__ void chunk_for(int64_t s0, int64_t e0, bool vec, F4&& f4, F1&& f1) {
    int64_t t0 = s0;
    if (vec) {
        const int64_t n4 = (e0 - s0) >> 2;
        for (int64_t j = threadIdx.x; j < n4; j += blockDim.x) f4(s0 + 4 * j);
        t0 = s0 + 4 * n4;
    }
    for (int64_t i = t0 + threadIdx.x; i < e0; i += blockDim.x) f1(i);
}
__device__ __forceinline__ bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The sum of a block's 256 doubles in a fixed order: a butterfly over each wave's 64 lanes (every lane forms the
// same tree), then the four wave sums in wave order.  Valid in thread 0.
__device__ __forceinline__ double block_sum_fixed(double s) {
    __shared__ double wave_sum[4];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
    __syncthreads();
    return ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

// grad *= inv_scale[0] with an inf / nan flag; NORM: plus the chunk's sum of squares of the unscaled gradients
// (fp64, every square exact) to partials[chunk].  NORM = false holds no LDS and no barrier.
template <bool NORM>
__global__ __launch_bounds__(256) void unscale_check_kernel(const ldm_tensor_slot* __restrict__ slots,
                                                            const int32_t* __restrict__ chunk_tensor,
                                                            const int64_t* __restrict__ chunk_start, int chunk_len,
                                                            const float* __restrict__ inv_scale,
                                                            int32_t* __restrict__ found_inf,
                                                            double* __restrict__ partials) {
    Chunk c;
    if (!chunk_open("unscale_check_kernel", slots, chunk_tensor, chunk_start, chunk_len, c)) return;
    const ldm_tensor_slot& sl = c.sl;
    const float is = inv_scale ? inv_scale[0] : 1.f;
    bool bad = false;
    double ss = 0.0;
    chunk_for(
        c.s0, c.e0, al16(sl.grad + c.s0),
        [&](int64_t i) {
            float4 g = *reinterpret_cast<const float4*>(sl.grad + i);
            g.x *= is, g.y *= is, g.z *= is, g.w *= is;
            *reinterpret_cast<float4*>(sl.grad + i) = g;
            bad |= !isfinite(g.x) || !isfinite(g.y) || !isfinite(g.z) || !isfinite(g.w);
            if constexpr (NORM) {
                ss += (double)g.x * (double)g.x;
                ss += (double)g.y * (double)g.y;
                ss += (double)g.z * (double)g.z;
                ss += (double)g.w * (double)g.w;
            }
        },
        [&](int64_t i) {
            const float g = sl.grad[i] * is;
            sl.grad[i] = g;
            bad |= !isfinite(g);
            if constexpr (NORM) ss += (double)g * (double)g;
        });
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(found_inf, 1);   // a flag, not a sum: order-free
    if constexpr (NORM) {
        const double total = block_sum_fixed(ss);
        if (threadIdx.x == 0) partials[blockIdx.x] = total;
    }
}

// One block.  Thread t sums its run of ceil(n / 256) consecutive partials in ascending order, thread 0 then the
// 256 run sums in ascending order: the partials in ascending chunk order, associated by runs (n <= 256: strictly
// one after the other).  out[0] = norm, out[1] = torch's clip coefficient min(1, max_norm / (norm + 1e-6)).
__global__ __launch_bounds__(256) void grad_norm_finalize_kernel(const double* __restrict__ partials, int64_t n,
                                                                 double max_norm, float* __restrict__ out) {
    __shared__ double run_sum[256];
    const int64_t run = (n + 255) / 256;
    const int64_t a = (int64_t)threadIdx.x * run, b = min(a + run, n);
    double s = 0.0;
    for (int64_t i = a; i < b; ++i) s += partials[i];
    run_sum[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sum = 0.0;
    for (int t = 0; t < 256; ++t) sum += run_sum[t];
    const double norm = sqrt(sum);
    double coef = 1.0;
    if (max_norm > 0.0) {
        coef = max_norm / (norm + 1e-6);   // NaN stays NaN, +inf gives 0, as torch's clamp(max=1) leaves them
        if (coef > 1.0) coef = 1.0;
    }
    out[0] = (float)norm;
    out[1] = (float)coef;
}

struct AdamScalars {
    float one_m_beta1, beta2, one_m_beta2, eps, weight_decay, decay_mul, step_size, bc2_sqrt;
};
static_assert(sizeof(AdamScalars) == 8 * sizeof(float), "AdamScalars is 8 floats");
// torch/optim/adam.py (_single_tensor_adam / _multi_tensor_adam, non-capturable): python floats, i.e. doubles
// cast once to fp32 (1 - beta computed in double).  The host-step entries form them here on the host, the
// capturable ones in adam_prep_kernel from the device step count: the same expressions, so the same bits.
__host__ __device__ inline AdamScalars adam_scalars(double lr, double beta1, double beta2, double eps,
                                                    double weight_decay, int decoupled, double step) {
    const double bc1 = 1.0 - pow(beta1, step);
    const double bc2 = 1.0 - pow(beta2, step);
    AdamScalars k;
    k.one_m_beta1 = (float)(1.0 - beta1);
    k.beta2 = (float)beta2;
    k.one_m_beta2 = (float)(1.0 - beta2);
    k.eps = (float)eps;
    k.weight_decay = (float)weight_decay;
    k.decay_mul = decoupled ? (float)(1.0 - lr * weight_decay) : 1.f;
    k.step_size = (float)(lr / bc1);
    k.bc2_sqrt = (float)sqrt(bc2);
    return k;
}

// Capturable step (hipGraph replay): the step count lives on the device and advances only on applied
// steps (found_inf clear), and the derived scalars are formed from it exactly as the host form forms them
// (double, one cast to fp32), so graphed and eager steps are bitwise equal.
__global__ void adam_prep_kernel(float* step, const int32_t* found_inf, double lr, double beta1, double beta2,
                                 double eps, double weight_decay, int decoupled, AdamScalars* out) {
    if (found_inf && found_inf[0]) return;
    const float st = step[0] + 1.f;
    step[0] = st;
    *out = adam_scalars(lr, beta1, beta2, eps, weight_decay, decoupled, (double)st);
}

// torch.optim.Adam / AdamW (_single_tensor_adam, non-capturable) on one element
__device__ __forceinline__ void adam_elem(const AdamScalars& k, float& p, float g, float& m, float& v) {
    if (k.decay_mul != 1.f) p = p * k.decay_mul;                 // AdamW: param.mul_(1 - lr * weight_decay)
    else if (k.weight_decay != 0.f) g = g + k.weight_decay * p;  // Adam: grad.add(param, alpha=wd)
    m = m + k.one_m_beta1 * (g - m);                              // exp_avg.lerp_(grad, 1 - beta1)
    v = v * k.beta2;                                              // exp_avg_sq.mul_(beta2)
    v = v + (k.one_m_beta2 * g) * g;                              //   .addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(v) / k.bc2_sqrt + k.eps;
    p = p + (-k.step_size) * (m / denom);                         // param.addcdiv_(exp_avg, denom, value=-step_size)
}

// a * b rounded to fp32 on its own: never contracted into a following add or subtract, so that a gradient
// multiplied in registers is bitwise the gradient that the same multiply wrote to memory
__device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

// e <- e + a (p - e) as one fused multiply-add, the same instruction in the fused and the stand-alone kernel
__device__ __forceinline__ void ema_elem(float& e, float p, float a) { e = __builtin_fmaf(a, p - e, e); }

// The Adam update of a chunk, skipped on inf/nan as GradScaler.step skips it.  kdev (capturable form): the
// scalars of the device-side step count, in place of k.  MUL: g <- g * grad_mul[0] in registers (a clip
// coefficient; .grad is not rewritten).  EMA: e <- e + one_m_decay (p_new - e), p_new still in registers.
template <bool MUL, bool EMA>
__global__ __launch_bounds__(256) void adam_kernel(const ldm_tensor_slot* __restrict__ slots,
                                                   const int32_t* __restrict__ chunk_tensor,
                                                   const int64_t* __restrict__ chunk_start, int chunk_len,
                                                   AdamScalars k, const int32_t* __restrict__ found_inf,
                                                   const AdamScalars* __restrict__ kdev,
                                                   const float* __restrict__ grad_mul, float* const* __restrict__ ema,
                                                   float one_m_decay) {
    if (found_inf && found_inf[0]) return;
    if (kdev) k = *kdev;
    Chunk c;
    if (!chunk_open("adam_kernel", slots, chunk_tensor, chunk_start, chunk_len, c)) return;
    const ldm_tensor_slot& sl = c.sl;
    const int64_t s0 = c.s0;
    const float gm = MUL ? grad_mul[0] : 1.f;
    float* const ev = EMA ? ema[c.ti] : nullptr;
    const bool vec = al16(sl.grad + s0) && al16(sl.param + s0) && al16(sl.exp_avg + s0) && al16(sl.exp_avg_sq + s0) &&
                     (!EMA || al16(ev + s0));
    chunk_for(
        s0, c.e0, vec,
        [&](int64_t i) {
            float4 g = *reinterpret_cast<const float4*>(sl.grad + i);
            float4 p = *reinterpret_cast<const float4*>(sl.param + i);
            float4 m = *reinterpret_cast<const float4*>(sl.exp_avg + i);
            float4 v = *reinterpret_cast<const float4*>(sl.exp_avg_sq + i);
            float4 e;
            if (EMA) e = *reinterpret_cast<const float4*>(ev + i);
            if (MUL) g.x = mul_rounded(g.x, gm), g.y = mul_rounded(g.y, gm), g.z = mul_rounded(g.z, gm), g.w = mul_rounded(g.w, gm);
            adam_elem(k, p.x, g.x, m.x, v.x);
            adam_elem(k, p.y, g.y, m.y, v.y);
            adam_elem(k, p.z, g.z, m.z, v.z);
            adam_elem(k, p.w, g.w, m.w, v.w);
            *reinterpret_cast<float4*>(sl.exp_avg + i) = m;
            *reinterpret_cast<float4*>(sl.exp_avg_sq + i) = v;
            *reinterpret_cast<float4*>(sl.param + i) = p;
            if (EMA) {
                ema_elem(e.x, p.x, one_m_decay);
                ema_elem(e.y, p.y, one_m_decay);
                ema_elem(e.z, p.z, one_m_decay);
                ema_elem(e.w, p.w, one_m_decay);
                *reinterpret_cast<float4*>(ev + i) = e;
            }
        },
        [&](int64_t i) {
            float p = sl.param[i], m = sl.exp_avg[i], v = sl.exp_avg_sq[i];
            float g = sl.grad[i];
            if (MUL) g = mul_rounded(g, gm);
            adam_elem(k, p, g, m, v);
            sl.exp_avg[i] = m;
            sl.exp_avg_sq[i] = v;
            sl.param[i] = p;
            if (EMA) {
                float e = ev[i];
                ema_elem(e, p, one_m_decay);
                ev[i] = e;
            }
        });
}

// The EMA update alone: slot.param the EMA tensor, slot.grad the tensor it follows
__global__ __launch_bounds__(256) void ema_update_kernel(const ldm_tensor_slot* __restrict__ slots,
                                                         const int32_t* __restrict__ chunk_tensor,
                                                         const int64_t* __restrict__ chunk_start, int chunk_len,
                                                         float one_m_decay, const int32_t* __restrict__ found_inf) {
    if (found_inf && found_inf[0]) return;
    Chunk c;
    if (!chunk_open("ema_update_kernel", slots, chunk_tensor, chunk_start, chunk_len, c)) return;
    const ldm_tensor_slot& sl = c.sl;
    chunk_for(
        c.s0, c.e0, al16(sl.grad + c.s0) && al16(sl.param + c.s0),
        [&](int64_t i) {
            const float4 p = *reinterpret_cast<const float4*>(sl.grad + i);
            float4 e = *reinterpret_cast<const float4*>(sl.param + i);
            ema_elem(e.x, p.x, one_m_decay);
            ema_elem(e.y, p.y, one_m_decay);
            ema_elem(e.z, p.z, one_m_decay);
            ema_elem(e.w, p.w, one_m_decay);
            *reinterpret_cast<float4*>(sl.param + i) = e;
        },
        [&](int64_t i) {
            float e = sl.param[i];
            ema_elem(e, sl.grad[i], one_m_decay);
            sl.param[i] = e;
        });
}

// torch.amp.GradScaler._amp_update_scale_: backoff on inf, grow after growth_interval clean steps
__global__ void update_scale_kernel(float* scale, int32_t* growth_tracker, const int32_t* found_inf,
                                    float growth_factor, float backoff_factor, int growth_interval) {
    if (found_inf[0]) {
        scale[0] = scale[0] * backoff_factor;
        growth_tracker[0] = 0;
    } else {
        const int successful = growth_tracker[0] + 1;
        if (successful == growth_interval) {
            scale[0] = scale[0] * growth_factor;
            growth_tracker[0] = 0;
        } else {
            growth_tracker[0] = successful;
        }
    }
}

}  // namespace ldm

using namespace ldm;

// ldm_unscale_check (partials NULL) and ldm_unscale_check_norm: `bad` is the calling entry's own message
static int unscale_launch(const char* bad, const ldm_tensor_slot* slots, const int32_t* chunk_tensor,
                          const int64_t* chunk_start, int32_t nchunks, int32_t chunk_len, const float* inv_scale,
                          int32_t* found_inf, double* partials, void* stream) {
    LDM_REQUIRE(slots && chunk_tensor && chunk_start && found_inf && nchunks >= 0, bad);
    if (nchunks == 0) return 0;
    const auto kernel = partials ? unscale_check_kernel<true> : unscale_check_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, slots, chunk_tensor, chunk_start,
                       chunk_len, inv_scale, found_inf, partials);
    LDM_CHECK_LAUNCH("unscale_check_kernel");
    return 0;
}

extern "C" int ldm_unscale_check(const ldm_tensor_slot* slots, const int32_t* chunk_tensor, const int64_t* chunk_start,
                                 int32_t nchunks, int32_t chunk_len, const float* inv_scale, int32_t* found_inf,
                                 void* stream) {
    return unscale_launch("unscale_check: bad argument", slots, chunk_tensor, chunk_start, nchunks, chunk_len, inv_scale,
                          found_inf, nullptr, stream);
}

extern "C" int ldm_unscale_check_norm(const ldm_tensor_slot* slots, const int32_t* chunk_tensor,
                                      const int64_t* chunk_start, int32_t nchunks, int32_t chunk_len,
                                      const float* inv_scale, int32_t* found_inf, double* partials, void* stream) {
    LDM_REQUIRE(partials && chunk_len > 0, "unscale_check_norm: bad argument");
    LDM_REQUIRE(((uintptr_t)partials & 7) == 0, "unscale_check_norm: partials must be 8-byte aligned");
    return unscale_launch("unscale_check_norm: bad argument", slots, chunk_tensor, chunk_start, nchunks, chunk_len,
                          inv_scale, found_inf, partials, stream);
}

extern "C" int ldm_grad_norm_finalize(const double* partials, int64_t nchunks, double max_norm, float* out,
                                      void* stream) {
    LDM_REQUIRE(out && nchunks >= 0 && (partials || nchunks == 0), "grad_norm_finalize: bad argument");
    LDM_REQUIRE(((uintptr_t)partials & 7) == 0, "grad_norm_finalize: partials must be 8-byte aligned");
    LDM_REQUIRE(max_norm == max_norm, "grad_norm_finalize: max_norm is NaN");
    hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, nchunks, max_norm,
                       out);
    LDM_CHECK_LAUNCH("grad_norm_finalize_kernel");
    return 0;
}

// The four ldm_adam_step* entries (`bad` is the calling entry's own message).  dev_step NULL: the scalars of the
// host step count `step`, as a kernel argument.  Otherwise adam_prep_kernel advances dev_step[0] and leaves its
// scalars in `scalars` (also for an empty chunk map), and the update reads them there.  ext NULL or empty: the
// plain update.
static int adam_launch(const char* bad, const ldm_tensor_slot* slots, const int32_t* chunk_tensor,
                       const int64_t* chunk_start, int32_t nchunks, int32_t chunk_len, double lr, double beta1,
                       double beta2, double eps, double weight_decay, int32_t decoupled, int32_t step, float* dev_step,
                       float* scalars, const int32_t* found_inf, const ldm_adam_ext* ext, void* stream) {
    LDM_REQUIRE(slots && chunk_tensor && chunk_start && nchunks >= 0, bad);
    hipStream_t st = (hipStream_t)stream;
    AdamScalars k{};
    const AdamScalars* kdev = nullptr;
    if (dev_step) {
        kdev = reinterpret_cast<const AdamScalars*>(scalars);
        hipLaunchKernelGGL(adam_prep_kernel, dim3(1), dim3(1), 0, st, dev_step, found_inf, lr, beta1, beta2, eps,
                           weight_decay, (int)decoupled, reinterpret_cast<AdamScalars*>(scalars));
        LDM_CHECK_LAUNCH("adam_prep_kernel");
    } else {
        k = adam_scalars(lr, beta1, beta2, eps, weight_decay, decoupled, (double)step);
    }
    if (nchunks == 0) return 0;
    const float* gm = ext ? ext->grad_mul : nullptr;
    float* const* ema = ext ? ext->ema : nullptr;
    float omd = 0.f;
    if (ema) {
        LDM_REQUIRE(ext->ema_decay >= 0.0 && ext->ema_decay < 1.0, "adam_step_ext: ema_decay must lie in [0, 1)");
        omd = (float)(1.0 - ext->ema_decay);
    }
    const auto kernel = gm ? (ema ? adam_kernel<true, true> : adam_kernel<true, false>)
                           : (ema ? adam_kernel<false, true> : adam_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(nchunks), dim3(256), 0, st, slots, chunk_tensor, chunk_start, chunk_len, k,
                       found_inf, kdev, gm, ema, omd);
    LDM_CHECK_LAUNCH("adam_kernel");
    return 0;
}

extern "C" int ldm_adam_step(const ldm_tensor_slot* slots, const int32_t* chunk_tensor, const int64_t* chunk_start,
                             int32_t nchunks, int32_t chunk_len, double lr, double beta1, double beta2, double eps,
                             double weight_decay, int32_t decoupled, int32_t step, const int32_t* found_inf,
                             void* stream) {
    LDM_REQUIRE(step >= 1, "adam_step: bad argument");
    return adam_launch("adam_step: bad argument", slots, chunk_tensor, chunk_start, nchunks, chunk_len, lr, beta1, beta2,
                       eps, weight_decay, decoupled, step, nullptr, nullptr, found_inf, nullptr, stream);
}

extern "C" int ldm_adam_step_dev(const ldm_tensor_slot* slots, const int32_t* chunk_tensor, const int64_t* chunk_start,
                                 int32_t nchunks, int32_t chunk_len, double lr, double beta1, double beta2, double eps,
                                 double weight_decay, int32_t decoupled, float* step, const int32_t* found_inf,
                                 float* scalars, void* stream) {
    LDM_REQUIRE(step && scalars, "adam_step_dev: bad argument");
    return adam_launch("adam_step_dev: bad argument", slots, chunk_tensor, chunk_start, nchunks, chunk_len, lr, beta1,
                       beta2, eps, weight_decay, decoupled, 0, step, scalars, found_inf, nullptr, stream);
}

extern "C" int ldm_adam_step_ext(const ldm_tensor_slot* slots, const int32_t* chunk_tensor, const int64_t* chunk_start,
                                 int32_t nchunks, int32_t chunk_len, double lr, double beta1, double beta2, double eps,
                                 double weight_decay, int32_t decoupled, int32_t step, const int32_t* found_inf,
                                 const ldm_adam_ext* ext, void* stream) {
    LDM_REQUIRE(step >= 1, "adam_step_ext: bad argument");
    return adam_launch("adam_step_ext: bad argument", slots, chunk_tensor, chunk_start, nchunks, chunk_len, lr, beta1,
                       beta2, eps, weight_decay, decoupled, step, nullptr, nullptr, found_inf, ext, stream);
}

extern "C" int ldm_adam_step_dev_ext(const ldm_tensor_slot* slots, const int32_t* chunk_tensor,
                                     const int64_t* chunk_start, int32_t nchunks, int32_t chunk_len, double lr,
                                     double beta1, double beta2, double eps, double weight_decay, int32_t decoupled,
                                     float* step, const int32_t* found_inf, float* scalars, const ldm_adam_ext* ext,
                                     void* stream) {
    LDM_REQUIRE(step && scalars, "adam_step_dev_ext: bad argument");
    return adam_launch("adam_step_dev_ext: bad argument", slots, chunk_tensor, chunk_start, nchunks, chunk_len, lr,
                       beta1, beta2, eps, weight_decay, decoupled, 0, step, scalars, found_inf, ext, stream);
}

extern "C" int ldm_ema_update(const ldm_tensor_slot* slots, const int32_t* chunk_tensor, const int64_t* chunk_start,
                              int32_t nchunks, int32_t chunk_len, double decay, const int32_t* found_inf,
                              void* stream) {
    LDM_REQUIRE(slots && chunk_tensor && chunk_start && nchunks >= 0 && chunk_len > 0, "ema_update: bad argument");
    LDM_REQUIRE(decay >= 0.0 && decay < 1.0, "ema_update: decay must lie in [0, 1)");
    if (nchunks == 0) return 0;
    hipLaunchKernelGGL(ema_update_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, slots, chunk_tensor,
                       chunk_start, chunk_len, (float)(1.0 - decay), found_inf);
    LDM_CHECK_LAUNCH("ema_update_kernel");
    return 0;
}

extern "C" int ldm_update_scale(float* scale, int32_t* growth_tracker, const int32_t* found_inf, float growth_factor,
                                float backoff_factor, int32_t growth_interval, void* stream) {
    LDM_REQUIRE(scale && growth_tracker && found_inf, "update_scale: bad argument");
    hipLaunchKernelGGL(update_scale_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, scale, growth_tracker, found_inf,
                       growth_factor, backoff_factor, growth_interval);
    LDM_CHECK_LAUNCH("update_scale_kernel");
    return 0;
}
