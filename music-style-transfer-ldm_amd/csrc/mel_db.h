// The per-element fp32 arithmetic of the log-mel formats, shared by the kernels that must agree bitwise:
// audio.hip (power <-> dB), dataio.hip (dB <-> 8-bit pixel <-> [0,1]) and longform.hip (the windowed front end
// and the crossfade stitch, which fuse them).  One fp32 rounding per reference operation: no contraction.
#pragma once
#include "common.h"

namespace ldm {

// 10 log10(max(amin, mx)): the reference level of an item whose maximum is mx
__device__ __forceinline__ float db_ref(float mx, float amin) { return 10.0f * log10f(fmaxf(amin, mx)); }

// 10 log10(max(amin, p)) - ref, clamped below at -top_db when top_db >= 0
__device__ __forceinline__ float power_db1(float p, float amin, float top_db, float ref) {
#pragma clang fp contract(off)   // 10 log10(max) - ref must cancel exactly: the item's maximum is 0 dB
    float v = 10.0f * log10f(fmaxf(amin, p)) - ref;
    if (top_db >= 0.f) v = fmaxf(v, -top_db);   // the item's own maximum is 0 dB
    return v;
}

__device__ __forceinline__ float db_power1(float db) { return exp10f(0.1f * db); }

// uint8(clip((db + max_db) * (255 / max_db), 0, 255) + 0.5): numpy float32 arithmetic, truncating cast
__device__ __forceinline__ unsigned char quant1(float v, float max_db, float scale) {
#pragma clang fp contract(off)
    float s = v + max_db;
    s = s * scale;
    s = s < 0.f ? 0.f : (s > 255.f ? 255.f : s);
    s = s + 0.5f;
    return (unsigned char)(int)s;
}

// ToTensor: u8 / 255 in fp32
__device__ __forceinline__ float unit1(unsigned char u) { return (float)u / 255.0f; }

}  // namespace ldm
