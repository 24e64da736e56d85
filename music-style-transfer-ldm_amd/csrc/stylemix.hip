// Style mixing: the folded cross-attention over a key set longer than the query map (several style references
// stacked along the keys), with a per-key additive bias (log of each reference's weight; -inf removes a key).
//
//   out(q) = sum_s exp(q.k_s + bias_s) v_s / sum_s exp(q.k_s + bias_s)
//
// attention_folded's instances (misc.hip) hold all S keys of a head in LDS and stop at S = 64.  This kernel
// streams the keys in tiles of ST with an online softmax (running maximum m, running sum l, the output
// accumulators rescaled by exp(m_old - m_new) per tile), so S is unbounded and need not be a multiple of ST.
//
// One block = NW waves = 16 query rows of one (batch, head).  Per key tile:
//   A  scores  z^T kf: the E-long contraction is split over the NW waves as in attention_mfma_kernel (each wave
//      covers every 16x16 tile of the block over its E/NW slice, all operand loads in flight at once); partial
//      tiles go to NW LDS slabs Sc.  z's fragments are loaded once, before the first tile.  The tile's V rows are
//      loaded to registers here too, and written to LDS after the barrier (the previous tile's P V still reads Vs).
//   B  softmax: one lane per key, rows over the waves: sums the slabs in wave order, adds bf (+ key_bias), updates
//      m and l (registers: a row always lands on the same lanes), writes p = exp(x - m) to Pn and the row's
//      rescale factor to Al.  The reference-bias form (RB, the style map) adds ref_bias[b][row][ref(s)] to the
//      lane's bias per row: loaded in A with the other operands, so B waits on nothing new.
//   C  O = O * alpha + V P^T on fp32 MFMA 16x16x4: channel tiles round-robin over the waves, accumulators in
//      registers across all key tiles; the division by l happens once, at the store.
// A key tile (or the leading tiles) may be entirely -inf: m stays -inf, and exp's argument is taken against 0
// instead (p = exp(-inf) = 0, alpha = exp(-inf) = 0), so no -inf - -inf is ever formed.
//
// LDS (static, 38 KB for either instance; the 64 KB a block gets without opting in is not exceeded):
//   Sc [NW][16][ST+4]  Pn [16][ST+2]  Vs [D][ST+2]  Al, Ls [16]
// Banks (ds_read_b32 / ds_write_b32: bank = dword address mod 32, conflicts within a 32-lane half):
//   Sc writes: lane (col, lg) stores row 4 lg + r, column col.  A half holds lg = {0,1} or {2,3}: the two groups
//      are 4 (ST+4) dwords apart = 16 mod 32 (ST = 32: 144, ST = 64: 272), each covers 16 consecutive banks:
//      conflict-free.  (Pitch ST+1, as the resident kernel has, puts them 4 banks apart: 2-way on 12 banks.)
//   Sc reads / Pn writes (softmax): a half walks 32 consecutive dwords of one row: conflict-free.
//   Vs writes: a half writes 32 consecutive keys of one channel row: conflict-free.
//   Vs / Pn reads (P V operands): lane (col, lg) reads row col, column 4 k + lg.  Pitch ST+2 = 2 mod 32, so a
//      half (col 0..15, lg in a pair) hits banks 2 col + lg (+ const): 32 distinct banks, conflict-free.
//      (Pitch ST+1 maps (col, 1) and (col+1, 0) to one bank: 2-way.)
//   Al / Ls: 16 consecutive dwords, lanes of equal col read the same address (broadcast).
#include <cmath>

#include "common.h"

namespace ldm {

// RB: the reference-bias form.  ref_bias [Bm, L, R] (fp32, finite or -inf) is the log-weight of reference
// ref(s) = s / (S / R) at query position l; samples b >= Bm take none (the guided loop's base half).  Without RB the
// three trailing arguments are unused and the code below is what it was.
template <int D, int EQ, int ST, int NW, bool RB>
__global__ __launch_bounds__(64 * NW) void attention_folded_tiled_kernel(const float* __restrict__ z,
                                                                         const float* __restrict__ kv,
                                                                         const float* __restrict__ kf,
                                                                         const float* __restrict__ bf,
                                                                         const float* __restrict__ key_bias,
                                                                         float* __restrict__ out, int heads, int L, int S,
                                                                         const float* __restrict__ ref_bias, int R,
                                                                         int Bm) {
    constexpr int TILE = 16, NLG = 4, LT = 16;
    constexpr int NSTEP = EQ / NW / NLG;          // MFMA steps of one wave's slice of the score contraction
    constexpr int NTS = ST / TILE;                // score tiles per key tile
    constexpr int NTC = D / TILE;                 // output channel tiles
    constexpr int NTO = (NTC + NW - 1) / NW;      // ... per wave
    constexpr int LDSC = ST + 4, LDP = ST + 2, LDV = ST + 2;
    constexpr int NVR = D * ST / (64 * NW);       // V elements per thread per key tile
    constexpr int RPW = 64 / ST;                  // softmax rows per wave pass
    constexpr int NPASS = LT / (NW * RPW);
    static_assert(ST == 32 || ST == 64, "one softmax lane per key of the tile");
    static_assert(EQ % (NW * 16) == 0 && NSTEP + NTS * NSTEP <= 96, "score fragments");
    static_assert((D * ST) % (64 * NW) == 0 && LT % (NW * RPW) == 0 && D % TILE == 0, "tile split");
    __shared__ float Sc[NW * LT * LDSC];
    __shared__ float Pn[LT * LDP];
    __shared__ float Vs[D * LDV];
    __shared__ float Al[LT], Ls[LT];
    const int nlb = (L + LT - 1) / LT;
    const int l0 = (blockIdx.x % nlb) * LT;
    const int bh = blockIdx.x / nlb;
    const int h = bh % heads, b = bh / heads;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane % TILE, lg = lane / TILE;
    const int E = heads * D;
    const float* kb = kf + (size_t)bh * S * EQ;
    const float* vb = kv + ((size_t)b * 2 * E + E + (size_t)h * D) * S;
    const float* bfb = bf + (size_t)bh * S;
    const float* kbias = key_bias ? key_bias + (size_t)b * S : nullptr;
    const int kbase = wave * (EQ / NW);

    // z fragments: MFMA step j = 4 jj + i takes lane group lg's k = kbase + 16 jj + 4 lg + i (one 16-byte load
    // feeds 4 steps); rows past L read row 0 and are zeroed
    float av[NSTEP];
    {
        const int l = l0 + col;
        const float4* zp = reinterpret_cast<const float4*>(z + ((size_t)b * L + (l < L ? l : 0)) * EQ + kbase + 4 * lg);
#pragma unroll
        for (int jj = 0; jj < NSTEP / 4; ++jj) {
            const float4 v = zp[4 * jj];
            av[4 * jj + 0] = l < L ? v.x : 0.f;
            av[4 * jj + 1] = l < L ? v.y : 0.f;
            av[4 * jj + 2] = l < L ? v.z : 0.f;
            av[4 * jj + 3] = l < L ? v.w : 0.f;
        }
    }
    const int sub = lane / ST, s0 = lane % ST;   // softmax: row within the pass, key within the tile
    float mrun[NPASS], lrun[NPASS];
#pragma unroll
    for (int p = 0; p < NPASS; ++p) mrun[p] = -INFINITY, lrun[p] = 0.f;
    floatx4 acc[NTO];
#pragma unroll
    for (int i = 0; i < NTO; ++i) acc[i] = floatx4{0.f, 0.f, 0.f, 0.f};
    // reference bias: each softmax pass' row of ref_bias (rows past L read row L - 1: never stored); the whole block
    // is one sample, so whether it takes a bias is uniform
    [[maybe_unused]] const float* rbrow[NPASS];
    [[maybe_unused]] const bool rbon = RB && b < Bm;
    [[maybe_unused]] const int SR = RB ? S / R : 1;   // keys per reference
    if constexpr (RB) {
#pragma unroll
        for (int p = 0; p < NPASS; ++p) {
            const int l = l0 + (wave + NW * p) * RPW + sub;
            rbrow[p] = ref_bias + ((size_t)(rbon ? b : 0) * L + (l < L ? l : L - 1)) * R;
        }
    }

    for (int sb = 0; sb < S; sb += ST) {
        // ---- A: this tile's folded keys and values, every load in flight before the first MFMA
        float bv[NTS][NSTEP];
#pragma unroll
        for (int st = 0; st < NTS; ++st) {
            const int s = sb + st * TILE + col;
            const float4* kp = reinterpret_cast<const float4*>(kb + (size_t)(s < S ? s : 0) * EQ + kbase + 4 * lg);
#pragma unroll
            for (int jj = 0; jj < NSTEP / 4; ++jj) {
                const float4 v = kp[4 * jj];
                bv[st][4 * jj + 0] = s < S ? v.x : 0.f;
                bv[st][4 * jj + 1] = s < S ? v.y : 0.f;
                bv[st][4 * jj + 2] = s < S ? v.z : 0.f;
                bv[st][4 * jj + 3] = s < S ? v.w : 0.f;
            }
        }
        float vr[NVR];
#pragma unroll
        for (int u = 0; u < NVR; ++u) {
            const int e = u * 64 * NW + (int)threadIdx.x;
            const int c = e / ST, s = sb + e % ST;
            const float v = vb[s < S ? (size_t)c * S + s : 0];
            vr[u] = s < S ? v : 0.f;   // a masked key's value is 0, never whatever lies there: its p is 0
        }
        float xb;   // the softmax lane's bias: bf (+ key_bias); keys past S are masked
        {
            const int s = sb + s0;
            xb = s < S ? bfb[s] + (kbias ? kbias[s] : 0.f) : -INFINITY;
        }
        [[maybe_unused]] float rb[NPASS];   // per row: the bias of this lane's key's reference (keys past S read the last)
        if constexpr (RB) {
#pragma unroll
            for (int p = 0; p < NPASS; ++p) rb[p] = 0.f;
            if (rbon) {
                const int s = sb + s0;
                const int ref = (s < S ? s : S - 1) / SR;
#pragma unroll
                for (int p = 0; p < NPASS; ++p) rb[p] = rbrow[p][ref];
            }
        }
        float* Sw = Sc + wave * LT * LDSC;
#pragma unroll
        for (int st = 0; st < NTS; ++st) {
            floatx4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < NSTEP; ++j) a = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bv[st][j], a, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) Sw[(4 * lg + r) * LDSC + st * TILE + col] = a[r];
        }
        __syncthreads();
        // ---- B: values to LDS, online softmax of the tile
#pragma unroll
        for (int u = 0; u < NVR; ++u) {
            const int e = u * 64 * NW + (int)threadIdx.x;
            Vs[(e / ST) * LDV + e % ST] = vr[u];
        }
#pragma unroll
        for (int p = 0; p < NPASS; ++p) {
            const int r = (wave + NW * p) * RPW + sub;
            float x = Sc[r * LDSC + s0];
#pragma unroll
            for (int w = 1; w < NW; ++w) x = x + Sc[w * LT * LDSC + r * LDSC + s0];
            if constexpr (RB) x += rbon ? xb + rb[p] : xb;
            else x += xb;
            float mx = x;
#pragma unroll
            for (int o = ST / 2; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
            const float mnew = fmaxf(mrun[p], mx);
            const float ms = mnew == -INFINITY ? 0.f : mnew;
            const float pv = expf(x - ms);
            const float alpha = expf(mrun[p] - ms);
            float sum = pv;
#pragma unroll
            for (int o = ST / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
            lrun[p] = lrun[p] * alpha + sum;
            mrun[p] = mnew;
            Pn[r * LDP + s0] = pv;
            if (s0 == 0) Al[r] = alpha;
        }
        __syncthreads();
        // ---- C: O[c][l] = O[c][l] alpha[l] + sum_s V[c][s] p[l][s]
#pragma unroll
        for (int i = 0; i < NTO; ++i) {
            const int ct = wave + NW * i;
            if (ct < NTC) {
                const float alpha = Al[col];
                floatx4 a = acc[i];
#pragma unroll
                for (int r = 0; r < 4; ++r) a[r] *= alpha;
                const float* va = Vs + (ct * TILE + col) * LDV + lg;
                const float* pb = Pn + col * LDP + lg;
#pragma unroll
                for (int k = 0; k < ST / NLG; ++k)
                    a = __builtin_amdgcn_mfma_f32_16x16x4f32(va[NLG * k], pb[NLG * k], a, 0, 0, 0);
                acc[i] = a;
            }
        }
        // no barrier here: the next tile writes Sc (last read in B, before the second barrier) and, after its own
        // first barrier, Vs / Pn / Al (every wave has left C by then)
    }
#pragma unroll
    for (int p = 0; p < NPASS; ++p)
        if (s0 == 0) Ls[(wave + NW * p) * RPW + sub] = lrun[p];
    __syncthreads();
    const int l = l0 + col;
    const float lsum = Ls[col];
    const float inv = lsum > 0.f ? 1.f / lsum : 0.f;   // every key masked: 0, not NaN
#pragma unroll
    for (int i = 0; i < NTO; ++i) {
        const int ct = wave + NW * i;
        if (ct < NTC && l < L)   // rows 4 lg .. 4 lg + 3 = 4 consecutive channels of token l
            *reinterpret_cast<float4*>(out + ((size_t)b * L + l) * E + (size_t)h * D + ct * TILE + 4 * lg) =
                make_float4(acc[i][0] * inv, acc[i][1] * inv, acc[i][2] * inv, acc[i][3] * inv);
    }
}

// bf[b,h,s] += key_bias[b,s] (the bias folded into the folded keys' bias once per loop)
__global__ __launch_bounds__(256) void fold_key_bias_kernel(float* __restrict__ bf, const float* __restrict__ key_bias,
                                                            int heads, int S, int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int s = (int)(idx % S);
    const int64_t b = idx / S / heads;
    bf[idx] += key_bias[b * S + s];
}

// The folded attention for any L, S >= 1 with an optional key bias [B,S].  S == L without a bias is
// attention_folded itself (the LDS-resident instances, unchanged); everything else streams the keys.
int attention_folded_keys(const float* z, const float* kv, const float* kf, const float* bf, const float* key_bias,
                          float* out, int32_t B, int32_t E, int32_t heads, int32_t L, int32_t S, hipStream_t st) {
    LDM_REQUIRE(z && kv && kf && bf && out, "attention (folded, keys): null argument");
    LDM_REQUIRE(B > 0 && heads == 4 && L > 0 && S > 0 && (E == 256 || E == 512),
                "attention (folded, keys): instances for E 256 and 512 at 4 heads");
    if (!key_bias && S == L && L <= (E == 256 ? 64 : 32)) return attention_folded(z, kv, kf, bf, out, B, E, heads, L, S, st);
    LDM_REQUIRE((((uintptr_t)z | (uintptr_t)kf | (uintptr_t)out) & 15) == 0,
                "attention (folded, keys): z, kf and out must be 16-byte aligned");
    const int64_t blocks = (int64_t)B * heads * ((L + 15) / 16);
    LDM_REQUIRE(blocks < (int64_t)1 << 31, "attention (folded, keys): too many query tiles");
    if (E == 256)
        hipLaunchKernelGGL((attention_folded_tiled_kernel<64, 256, 64, 4, false>), dim3((unsigned)blocks), dim3(256), 0, st,
                           z, kv, kf, bf, key_bias, out, heads, L, S, nullptr, 0, 0);
    else
        hipLaunchKernelGGL((attention_folded_tiled_kernel<128, 512, 32, 8, false>), dim3((unsigned)blocks), dim3(512), 0, st,
                           z, kv, kf, bf, key_bias, out, heads, L, S, nullptr, 0, 0);
    LDM_CHECK_LAUNCH("attention_folded_tiled_kernel");
    return 0;
}

// The style map: attention_folded_keys with a per-(query position, reference) bias ref_bias [Bm, L, R] on top of the
// key bias; key s belongs to reference s / (S / R), samples b >= Bm take none.  ref_bias NULL (or Bm == 0) is
// attention_folded_keys itself.  Always the streaming kernel: the bias lives in its softmax phase.
int attention_folded_keys_map(const float* z, const float* kv, const float* kf, const float* bf, const float* key_bias,
                              const float* ref_bias, int32_t R, int32_t Bm, float* out, int32_t B, int32_t E, int32_t heads,
                              int32_t L, int32_t S, hipStream_t st) {
    if (!ref_bias || Bm == 0) return attention_folded_keys(z, kv, kf, bf, key_bias, out, B, E, heads, L, S, st);
    LDM_REQUIRE(z && kv && kf && bf && out, "attention (folded, map): null argument");
    LDM_REQUIRE(B > 0 && heads == 4 && L > 0 && S > 0 && (E == 256 || E == 512),
                "attention (folded, map): instances for E 256 and 512 at 4 heads");
    LDM_REQUIRE(R >= 1 && S % R == 0, "attention (folded, map): the key count must be a multiple of the reference count");
    LDM_REQUIRE(Bm > 0 && Bm <= B, "attention (folded, map): the biased sample count must lie in [0, B]");
    LDM_REQUIRE((((uintptr_t)z | (uintptr_t)kf | (uintptr_t)out) & 15) == 0,
                "attention (folded, map): z, kf and out must be 16-byte aligned");
    const int64_t blocks = (int64_t)B * heads * ((L + 15) / 16);
    LDM_REQUIRE(blocks < (int64_t)1 << 31, "attention (folded, map): too many query tiles");
    if (E == 256)
        hipLaunchKernelGGL((attention_folded_tiled_kernel<64, 256, 64, 4, true>), dim3((unsigned)blocks), dim3(256), 0, st,
                           z, kv, kf, bf, key_bias, out, heads, L, S, ref_bias, R, Bm);
    else
        hipLaunchKernelGGL((attention_folded_tiled_kernel<128, 512, 32, 8, true>), dim3((unsigned)blocks), dim3(512), 0, st,
                           z, kv, kf, bf, key_bias, out, heads, L, S, ref_bias, R, Bm);
    LDM_CHECK_LAUNCH("attention_folded_tiled_kernel (map)");
    return 0;
}

// attention_fold_keys, then the key bias added to bf.  key_bias NULL: attention_fold_keys alone.
int attention_fold_keys_bias(const float* kv, const float* wq, const float* bq, int32_t B, int32_t E, int32_t heads,
                             int32_t S, float scale, const float* key_bias, float* kf, float* bf, hipStream_t st) {
    int rc = attention_fold_keys(kv, wq, bq, B, E, heads, S, scale, kf, bf, st);
    if (rc || !key_bias) return rc;
    const int64_t n = (int64_t)B * heads * S;
    hipLaunchKernelGGL(fold_key_bias_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, bf, key_bias, heads, S, n);
    LDM_CHECK_LAUNCH("fold_key_bias_kernel");
    return 0;
}

}  // namespace ldm

extern "C" int ldm_attention_folded_keys(const float* z, const float* kv, const float* kf, const float* bf,
                                         const float* key_bias, float* out, int32_t B, int32_t E, int32_t heads,
                                         int32_t L, int32_t S, void* stream) {
    return ldm::attention_folded_keys(z, kv, kf, bf, key_bias, out, B, E, heads, L, S, (hipStream_t)stream);
}

extern "C" int ldm_attention_folded_keys_map(const float* z, const float* kv, const float* kf, const float* bf,
                                             const float* key_bias, const float* ref_bias, int32_t R, int32_t Bm,
                                             float* out, int32_t B, int32_t E, int32_t heads, int32_t L, int32_t S,
                                             void* stream) {
    return ldm::attention_folded_keys_map(z, kv, kf, bf, key_bias, ref_bias, R, Bm, out, B, E, heads, L, S,
                                          (hipStream_t)stream);
}

extern "C" int ldm_attention_fold_keys_bias(const float* kv, const float* wq, const float* bq, int32_t B, int32_t E,
                                            int32_t heads, int32_t S, float scale, const float* key_bias, float* kf,
                                            float* bf, void* stream) {
    return ldm::attention_fold_keys_bias(kv, wq, bq, B, E, heads, S, scale, key_bias, kf, bf, (hipStream_t)stream);
}
