// Step kernels of the reverse loop: the nine convolutions of UNet.forward (model.py:178-194, :205-229)
// as fixed-structure implicit GEMMs for gfx950, used by ldm_sample when use_step != 0.
//
// Why a second conv family next to conv.hip: at the sampling batch (B = 8 on a 16x64 latent) every layer
// is a 0.3-0.6 GFLOP GEMM whose output is only 64K-512K values, so a launch is ~256 blocks that each own
// one output tile and split K over their waves.  conv.hip's general kernel (runtime tap tables, phase
// tables, K cursors, split-K hand-off) spends most of such a launch on dependent operand rounds and
// address arithmetic.  Here the channel counts, the tap structure and the per-wave K range are template
// constants, so:
//   * the K order is channel-chunk major, tap minor (chunk c = cc*9 + tap): a wave's chunk range is a
//     whole number of channel chunks times the 9 taps, every chunk's tap is a compile-time constant, and
//     the per-lane input offset of each tap is computed once — the K loop is loads + MFMAs only;
//   * every operand load of a stage is issued before the first MFMA of that stage (one memory round trip
//     per stage; most layers are a single stage, so the whole K range is in flight at once);
//   * activations are NHWC: a lane's 4 channels of a 16-channel chunk are one 16-byte load, and the
//     16x16 accumulator rows of a lane (4 consecutive output channels) are one 16-byte store.
// The stride-2 transposed convolutions (dec4..dec2) run over the INPUT grid with 4 accumulator sets, one
// per output parity: tap (ky, kx) of ConvTranspose2d(k3, s2, p1, op1) reads input (qy + [ky==0],
// qx + [kx==0]) and feeds output (2qy + [ky!=1], 2qx + [kx!=1]) — every block carries the same 9-tap K,
// so the four parities need no separate (unequal) launches.
//
// MFMA: v_mfma_f32_16x16x4_f32 (exact fp32, = an fmaf chain, cdna_hip_programming.md §3).  Lane l holds
// A[row = l & 15][k] and B[k][col = l & 15] for its lane group lg = l >> 4; within a 16-channel chunk,
// MFMA step j uses k-local channel 4*lg + j.  D: row 4*lg + r, col l & 15.
// Summation order differs from torch's (K blocked over waves, fixed order), well inside 1e-4.
#include <algorithm>
#include <cstdlib>

#include "uconv_kernel.h"

namespace ldm {
namespace uc {

// packed[c][m][16], c = cc*9 + t, element e = 4*lg + j  ->  input channel cc*16 + e, tap t = ky*3 + kx.
// conv: w [COUT][CIN][3][3]; transposed conv: w [CIN][COUT][3][3] (torch layouts).  DT: element type of the
// pack (0 fp32; LDM_DT_F16 / LDM_DT_BF16: rounded once here, to nearest even, as the kernels would round it).
template <int DT>
__global__ __launch_bounds__(256) void uconv_pack_kernel(const float* __restrict__ w, void* __restrict__ outp,
                                                         int CIN, int COUT, int transposed) {
    const int64_t total = (int64_t)9 * CIN * COUT;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int e = (int)(idx % 16);
    const int m = (int)((idx / 16) % COUT);
    const int c = (int)(idx / (16 * (int64_t)COUT));
    const int cc = c / 9, t = c % 9;
    const int ci = cc * 16 + e;
    const float v = transposed ? w[((int64_t)ci * COUT + m) * 9 + t] : w[((int64_t)m * CIN + ci) * 9 + t];
    if constexpr (DT == 0)
        reinterpret_cast<float*>(outp)[idx] = v;
    else if constexpr (DT == LDM_DT_F16)
        reinterpret_cast<_Float16*>(outp)[idx] = (_Float16)v;
    else
        reinterpret_cast<__bf16*>(outp)[idx] = (__bf16)v;
}

// NCHW <-> NHWC for the sampler state (once before / after the loop)
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float* __restrict__ x, float* __restrict__ y, int C,
                                                           int HW, int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over y (NHWC)
    if (idx >= n) return;
    const int c = (int)(idx % C);
    const int64_t r = idx / C;
    const int p = (int)(r % HW);
    const int64_t b = r / HW;
    y[idx] = x[(b * C + c) * HW + p];
}
__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const float* __restrict__ x, float* __restrict__ y, int C,
                                                           int HW, int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over y (NCHW)
    if (idx >= n) return;
    const int p = (int)(idx % HW);
    const int64_t r = idx / HW;
    const int c = (int)(r % C);
    const int64_t b = r / C;
    y[idx] = x[(b * HW + p) * C + c];
}

// ------------------------------------------------------------------------------------------------------
// Layer table: the nine layers; the instance each runs is named in step_conv (the batch only changes the grid),
// chosen so that at the sampling batch (B = 8, 16x64 latent) a launch is 256 equal blocks (dec4: 128),
// one wave per SIMD (bottleneck / dec4: two) and 144 MFMAs per wave.
// ------------------------------------------------------------------------------------------------------
struct LayerGeo {
    int mode, cin, cout;   // (for the pack and the tensor sizes; an instance's tile shape is its launch<>'s, see set_grid)
};
constexpr LayerGeo kGeo[9] = {
    {0, 32, 64},     // enc1        conv3x3 s1
    {1, 64, 128},    // enc2        conv3x3 s2 (+ t_emb)
    {1, 128, 256},   // enc3        conv3x3 s2
    {1, 256, 512},   // enc4        conv3x3 s2 (folded with CA2's out-projection)
    {0, 512, 512},   // bottleneck  conv3x3 s1 (folded with CA1's out-projection)
    {2, 512, 256},   // dec4        convT k3 s2 (+ skip z3)
    {2, 256, 128},   // dec3        convT (+ skip z2)
    {2, 128, 64},    // dec2        convT (+ skip z1)
    {0, 64, 32},     // dec1        conv3x3 s1 (+ fused DDIM update)
};
// spatial size divisor of each layer's input (model.py:178-194)
constexpr int kDiv[9] = {1, 1, 2, 4, 8, 8, 4, 2, 1};

// The tables below size the split-K workspace (ks_tiles, step_ws_floats) and say which form a layer has (ks_form,
// step_ks_mask); the instance that runs is the one step_conv names, and set_grid checks its tile count against them.

// The K-split form of the deep layers (variant 1): a 32 x 32 block tile (2 x 2 MFMA tiles per wave) instead of
// 16 x 16, so a block pulls half the operand bytes per MFMA, with K split over KS blocks to keep 256 blocks
// (write-through partial tiles, last arriver sums in split order).  {tm, tn, wk, ks}; ks 0 = no variant.
struct KsGeo {
    int tm, tn, wk, ks, wn = 1;
};
constexpr KsGeo kKs[9] = {
    {0, 0, 0, 0},   // enc1
    {0, 0, 0, 0},   // enc2
    {2, 2, 4, 2},   // enc3        128 tiles x 2
    {2, 2, 4, 4},   // enc4        64 tiles x 4
    {2, 2, 8, 4},   // bottleneck  64 tiles x 4, 8 waves
    {2, 2, 4, 8},   // dec4        32 tiles x 8
    {2, 2, 4, 4},   // dec3        64 tiles x 4
    {0, 0, 0, 0},   // dec2
    {0, 0, 0, 0},   // dec1
};

// Variant 2 ("thin"): a 16 x 32 block tile with K split over 2-4 blocks of 8 waves: the same weight bytes per
// block as variant 1, a partial tile of a quarter / half the size for the last arriver to gather (its hand-off
// cost grows with KS x the tile).  Selected by bit l of LDM_UCONV_KS2 for a layer also in LDM_UCONV_KS.
constexpr KsGeo kKs2[9] = {
    {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0},
    {1, 2, 8, 2},   // enc4        128 tiles x 2
    {1, 2, 4, 4, 2},   // bottleneck  64 tiles (16 x 64: 2 wave columns) x 4, two channel chunks per wave
    {1, 2, 8, 4},   // dec4        64 tiles x 4
    {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0},
};

// Variant 3 ("wide", round 6): 16 x 16 tiles with one channel chunk per wave and 16 waves per block (4 per SIMD), so a
// block keeps 16 x 9 operand loads in flight across four times the waves: enc4 with K in one block (256 tiles, no
// partial slabs), dec4 with K over 2 blocks (128 tiles; half the slab bytes of variant 2).  Bit l of LDM_UCONV_KS3
// (default 0xED: every layer that has one; it takes precedence over LDM_UCONV_KS / _KS2 for that layer).  Measured
// in the fp32 loop (B = 8, one box each): none 75.28, enc4 73.47-73.68, dec4 74.28-74.37, both 72.21-72.69 us per
// iteration (gpurun_out/r6b7); then on another box from enc4 + dec4 (72.15-72.39): + enc1 71.59-71.74, + enc3
// 71.41-71.71, + dec3 71.44-71.56, + dec2 72.34-72.50, all six 70.12-70.18 (gpurun_out/r6b8); the fp16 loop
// 57.97 -> 56.70-57.06 with enc4 + dec4, unchanged by the other four; + dec1 with its DDIM update 70.30-70.44 ->
// 69.72-69.87, fp16 55.50-55.73 -> 55.19-55.23 (gpurun_out/r6b9).
// Round 7: dec4's two blocks per tile split the taps by output parity (kTapClass, dec4_par()) instead of K: no
// partial slabs, dec4 7.66 -> 6.35 us (rocprof average), WRITE 1.585 -> 0.524 MB per launch, the fp32 loop
// 69.76-69.96 -> 68.94-69.24, fp16 55.16-55.42 -> 53.90-54.30 us per iteration (profiles/r07).  The K-split row
// below stays selectable (LDM_UCONV_DEC4_PAR=0) and sizes the workspace.
constexpr KsGeo kKs3[9] = {
    {2, 1, 2, 1, 4},   // enc1        32 x 64 tiles (4 wave columns), K (2 channel chunks) over 2 waves: 8 waves
    {2, 1, 4, 1, 2},   // enc2        32 x 32 tiles (2 wave columns of 16), K over 4 waves: 8 waves
    {2, 1, 8, 1},    // enc3        32 x 16 tiles, K over 8 waves
    {1, 1, 16, 1},   // enc4        256 tiles, K whole
    {0, 0, 0, 0},
    {1, 1, 16, 2},   // dec4        128 tiles x 2 (K halves; by default the two tap classes instead)
    {1, 1, 16, 1},   // dec3        256 tiles, K over 16 waves
    {1, 2, 8, 1},    // dec2        16 x 32 tiles, K over 8 waves
    {1, 2, 4, 1, 2}, // dec1 + DDIM 16 x 64 tiles (2 wave columns), K over 4 waves: 8 waves
};
constexpr int kKs3Default = 0x1ED;   // enc1, enc3, enc4, dec4, dec3, dec2, dec1 (gpurun_out/r6b7, r6b8, r6b9)

// One LDM_UCONV_* variable (each is read once per process, into the static of its reader below).
static int env_int(const char* name, int dflt, int base = 10) {
    const char* e = std::getenv(name);
    return e ? (int)std::strtol(e, nullptr, base) : dflt;
}
static int ks3_mask() {
    static const int m = env_int("LDM_UCONV_KS3", kKs3Default, 0);
    return m;
}
// Layers that run the K-split variant: bit l of LDM_UCONV_KS (read once; default kKsDefault).
// Round 2, in the loop's chain timing (B = 8): the split form gained 0.4 us on the bottleneck and 0.2 us on enc4
// and lost 0.9-1.5 us on enc3, dec4 and dec3.  Round 3, with the taps formed from LDS windows, the loop with
// enc4, the bottleneck and dec4 split (enc4 and dec4 on the thin variant kKs2) measured best (79.7-79.9 us per
// iteration against 84.0 for the round-2 choice, profiles/r03/ks2, profiles/r03/geo).
constexpr int kKsDefault = (1 << 3) | (1 << 4) | (1 << 5);
static int ks_mask() {
    static const int m = env_int("LDM_UCONV_KS", kKsDefault, 0);
    return m;
}
// 16-bit operands (config 5) stream half the weight bytes per block, so the split that pays for fp32 need not pay
// there: their own mask, LDM_UCONV_KS_LOWP (default kKsDefaultLowp, measured in the fp16 loop)
constexpr int kKsDefaultLowp = kKsDefault;
static int ks_mask_lowp() {
    static const int m = env_int("LDM_UCONV_KS_LOWP", kKsDefaultLowp, 0);
    return m;
}
// (the bottleneck's variants measured alike: 16 x 32 KS 2 79.7, 16 x 64 KS 4 80.1, 32 x 32 KS 4 79.9 us per
// iteration, profiles/r03/geo; it keeps variant 1)
constexpr int kKs2Default = (1 << 3) | (1 << 5);
static int ks2_mask() {
    static const int m = env_int("LDM_UCONV_KS2", kKs2Default, 0);
    return m;
}
// dec1 on 16-row x 64-position tiles: half of the 32 output channels per block, so a block streams half of the
// layer's weights (every block streams all of them in the 32-row form): loop 81.2 -> 80.7 us per iteration
// (profiles/r03/dec1_thin); LDM_UCONV_DEC1_THIN=0 keeps the 32-row form
static bool dec1_thin(int W) {
    static const bool on = env_int("LDM_UCONV_DEC1_THIN", 1) != 0;
    return on && W % 32 == 0;
}
// enc2 on 16-row x 64-position tiles (four wave columns sharing each weight fragment through L1): half the weight
// bytes per block of the 32 x 32 form, measured slower in the loop (81.6 vs 80.1 us per iteration,
// profiles/r03/geo); LDM_UCONV_ENC2_WIDE=1 (A/B timing)
static bool enc2_wide(int W) {
    static const bool on = env_int("LDM_UCONV_ENC2_WIDE", 0) != 0;
    return on && (W / 2) % 16 == 0;
}
// enc3 on 16-row tiles (half the weight bytes per block of the 32-row form), each wave one 16-column row of the
// 4 x 16 output plane so that its taps come from a row window.  Measured in the loop: 80.9 against 80.5 us per
// iteration for the 32-row form (profiles/r03/enc3_thin), so off unless LDM_UCONV_ENC3_THIN=1.
static bool enc3_thin(int W) {
    static const bool on = env_int("LDM_UCONV_ENC3_THIN", 0) != 0;
    return on && (W / 4) % 16 == 0;   // enc3's output row (W / 4 columns) holds whole 16-column groups
}
// EPI_WINDOW instances where the geometry allows (LDM_UCONV_WINDOW=0 turns them off for A/B timing)
static bool window_taps() {
    static const bool on = env_int("LDM_UCONV_WINDOW", 1) != 0;
    return on;
}
// XCD-grid block order (order 2 in set_grid); LDM_UCONV_XCD=0 turns it off for A/B timing
bool xcd_grid() {
    static const bool on = env_int("LDM_UCONV_XCD", 1) != 0;
    return on;
}
// EPI_PLANE instances where the geometry allows (LDM_UCONV_PLANE=0 turns them off for A/B timing)
static bool plane_taps() {
    static const bool on = env_int("LDM_UCONV_PLANE", 1) != 0;
    return on;
}
// dec4's wide form split over two blocks by tap class (kTapClass) instead of by K; LDM_UCONV_DEC4_PAR=0 keeps the
// K-split instance (A/B timing)
static bool dec4_par() {
    static const bool on = env_int("LDM_UCONV_DEC4_PAR", 1) != 0;
    return on;
}

static bool ks_on(int layer, int dtype = LDM_DT_F32) {
    return kKs[layer].ks > 1 && (((dtype == LDM_DT_F32 ? ks_mask() : ks_mask_lowp()) >> layer) & 1);
}
// K-split form of a layer: 0 none, 1 variant 1 (kKs), 2 variant 2 (kKs2), 3 variant 3 (kKs3)
// (variant 3 runs at the canonical 16 x 64 latent only: enc4 / dec4 on its 2 x 8 planes (EPI_PLANE), the others on
// whole rows of their column grids (EPI_WINDOW))
static int ks_form(int layer, int dtype = LDM_DT_F32, int H = 16, int W = 64) {
    if (layer >= 0 && layer <= 8 && kKs3[layer].wk > 0 && ((ks3_mask() >> layer) & 1) && H == 16 && W == 64 &&
        (layer == 3 || layer == 5 ? plane_taps() : window_taps()))
        return 3;
    if (layer < 0 || layer > 8 || !ks_on(layer, dtype)) return 0;
    return (kKs2[layer].ks > 1 && ((ks2_mask() >> layer) & 1)) ? 2 : 1;
}
// the table row of K-split form `form` (1..3)
static const KsGeo& ks_row(int layer, int form) { return form == 3 ? kKs3[layer] : (form == 2 ? kKs2[layer] : kKs[layer]); }
static void ks_tiles(int layer, int B, int H, int W, int64_t& tiles, int64_t& slab_floats, int form = 1) {
    const LayerGeo& g = kGeo[layer];
    const KsGeo& k = ks_row(layer, form);
    const int Hin = H / kDiv[layer], Win = W / kDiv[layer];
    const int64_t nq = (int64_t)B * (g.mode == 1 ? (Hin / 2) * (Win / 2) : Hin * Win);
    tiles = (int64_t)(g.cout / (16 * k.tm)) * ((nq + 16 * k.tn * k.wn - 1) / (16 * k.tn * k.wn));
    slab_floats = tiles * k.ks * (g.mode == 2 ? 4 : 1) * k.tm * k.tn * k.wn * 256;
}
}  // namespace uc

// Packed floats of layer `layer`'s step weights (9*Cin*Cout).
int64_t step_packed_floats(int layer) {
    if (layer < 0 || layer > 8) return -1;
    return (int64_t)9 * uc::kGeo[layer].cin * uc::kGeo[layer].cout;
}

// Split-K workspace of the step kernels at this shape: arrival counters (one int32 per tile, zero between
// launches) sized for the layer with the most tiles, then the largest layer's partial slabs.
// the layers on a K-split form (ldm_step_layer_forms): LDM_UCONV_KS's, with the wide variant's layers counted by its
// own split (enc4's wide form keeps K in one block)
int step_ks_mask() {
    int m = uc::ks_mask();
    for (int l = 0; l < 9; ++l)
        if (uc::kKs3[l].wk > 0 && ((uc::ks3_mask() >> l) & 1))
            m = uc::kKs3[l].ks > 1 && !(l == 5 && uc::dec4_par()) ? (m | (1 << l)) : (m & ~(1 << l));
    return m;
}

int64_t step_ws_floats(int B, int H, int W, int64_t* cnt_floats) {
    using namespace uc;
    int64_t mt = 0, ms = 0;
    for (int l = 0; l < 9; ++l) {
        for (int form = 1; form <= 3; ++form) {   // every K-split geometry, whatever the masks select
            if ((form == 1 ? kKs[l].ks : (form == 2 ? kKs2[l].ks : kKs3[l].ks)) <= 1) continue;
            int64_t t, sf;
            ks_tiles(l, B, H, W, t, sf, form);
            mt = std::max(mt, t);
            ms = std::max(ms, sf);
        }
    }
    const int64_t c = (mt + 63) / 64 * 64;
    if (cnt_floats) *cnt_floats = c;
    return c + ms;
}


namespace uc {
// The launch arguments of layer `layer` that do not depend on the instance's tile shape (set_grid adds those).
static int make_args(int layer, int B, int H, int W, const StepConv& s, UArgs& a) {
    LDM_REQUIRE(layer >= 0 && layer <= 8, "step conv: layer index");
    LDM_REQUIRE(B > 0 && H % 8 == 0 && W % 8 == 0, "step conv: latent H, W must be multiples of 8");
    const LayerGeo& g = kGeo[layer];
    const int Hin = H / kDiv[layer], Win = W / kDiv[layer];
    a = UArgs{};
    a.x = s.x;
    a.w = s.w;
    a.y = s.y;
    a.bias = s.bias;
    a.bcast = s.bcast;
    a.skip = s.skip;
    a.coef = s.coef;
    a.xs = s.xs;
    a.x0_log = s.x0_log;
    a.eps_log = s.eps_log;
    a.eta = s.eta;
    a.x0_prev = s.x0_prev;
    if (s.guide_eb) a.skip = s.guide_eb, a.bcast = s.guide_scale, a.y = s.xs2;   // (EPI_GUIDE's slots, see UArgs)
    if (s.keep_base) a.skip = s.keep_base, a.bcast = s.keep_row;                 // (EPI_KEEP's, likewise)
    a.B = B;
    a.Hin = Hin;
    a.Win = Win;
    if (g.mode == 0) {
        a.Hout = Hin, a.Wout = Win, a.Hq = Hin, a.Wq = Win;
    } else if (g.mode == 1) {
        a.Hout = Hin / 2, a.Wout = Win / 2, a.Hq = a.Hout, a.Wq = a.Wout;
    } else {
        a.Hout = 2 * Hin, a.Wout = 2 * Win, a.Hq = Hin, a.Wq = Win;
    }
    a.Nq = B * a.Hq * a.Wq;
    a.fd_hw = FastDiv::make(a.Hq * a.Wq);
    a.fd_w = FastDiv::make(a.Wq);
    LDM_REQUIRE((int64_t)B * Hin * Win * g.cin * 4 < 0x7ff00000LL && (int64_t)B * a.Hout * a.Wout * g.cout * 4 < 0x7ff00000LL,
                "step conv: tensor too large for 32-bit buffer offsets");
    LDM_REQUIRE(s.x && s.w && s.bias, "step conv: null operand");
    LDM_REQUIRE(!s.msolver || (layer == 8 && s.x0_log), "step conv: the multistep update is dec1's and needs its x0 log");
    LDM_REQUIRE((!s.plain && !s.guide_eb) || layer == 8, "step conv: the guided loop's two launches are dec1's");
    LDM_REQUIRE(!s.plain || (s.y && !s.guide_eb), "step conv: dec1's base half is a plain conv into y");
    LDM_REQUIRE(!s.guide_eb || ((s.guide_scale || s.keep_base) && s.xs2 && s.xs2 != s.xs),
                "step conv: guidance needs its scales and second state");
    LDM_REQUIRE(!s.keep_base || (layer == 8 && !s.plain && s.keep_row && (!s.guide_eb || s.guide_eb == s.keep_base)),
                "step conv: the regional keep is dec1's and needs its region and row (e_b leading the region when guided)");
    // (the kernel finds z0 / n0 / w behind skip by its own launch shape: it must be the shape the region was laid out for)
    LDM_REQUIRE(!s.keep_base || (int64_t)a.B * a.Hout * a.Wout * g.cout == s.keep_stride,
                "step conv: the keep region was laid out for another batch or plane than this launch's");
    return 0;
}

// The workspace of form ksv of `layer` as the tables size it (empty where that form keeps K in one block).
static KsWs ks_ws(int layer, int B, int H, int W, int ksv, float* ws) {
    KsWs k;
    if (ksv && ks_row(layer, ksv).ks > 1) {
        k.ws = ws;
        k.ws_floats = step_ws_floats(B, H, W, &k.cnt_floats);
        ks_tiles(layer, B, H, W, k.tiles, k.slab_floats, ksv);
    }
    return k;
}

// The instance with the geometry flag FLAG (EPI_PLANE / EPI_WINDOW) where `on`, else without it.
template <int FLAG, int MODE, int CIN, int COUT, int TM, int TN, int WN, int WK, int NCH, int S, int EPI, int KS = 1>
static int launch_opt(bool on, const UArgs& a, int dtype, hipStream_t st, const KsWs& k = {}) {
    if (on) return launch<MODE, CIN, COUT, TM, TN, WN, WK, NCH, S, EPI | FLAG, KS>(a, dtype, st, k);
    return launch<MODE, CIN, COUT, TM, TN, WN, WK, NCH, S, EPI, KS>(a, dtype, st, k);
}

// dec1's geometry (the index of uconv_kernel.h's list); Wq: the width of its column grid
static int dec1_geo(int ksv, int W, int Wq) {
    if (ksv == 3) return 0;
    if (dec1_thin(W)) return window_taps() ? 1 : 2;
    return window_taps() && Wq % 32 == 0 ? 3 : 4;   // (window: a block's 32 columns lie in one row)
}
}  // namespace uc

int step_conv(int layer, int B, int H, int W, const StepConv& s, hipStream_t st) {
    using namespace uc;
    const int ksv = s.ws ? ks_form(layer, s.dtype, H, W) : 0;   // without a workspace: the single-block form
    UArgs a;
    if (int rc = make_args(layer, B, H, W, s, a)) return rc;
    const KsWs k = ks_ws(layer, B, H, W, ksv, s.ws);
    const int dt = s.dtype;
    const bool win = window_taps();
    // EPI_PLANE where the layer's plane is the canonical one: a 2 x 8 plane, read by enc4 from a 4 x 16 input
    const bool pl28 = a.Hin == 2 && a.Win == 8 && plane_taps(), pl416 = a.Hin == 4 && a.Win == 16 && plane_taps();
    // dec1: its geometry, then the epilogue its caller asks for.  The plain DDIM / multistep instances are named among
    // the cases below (variant 3's with the other variant-3 layers, the rest last): that is the order of the kernels in
    // the code object, which is left as it was measured.
    int geo = 0;
    auto dec1_ms = [&](auto g) { return dec1_launch<EPI_MSOLVER, decltype(g)::value>(a, dt, st); };
    auto dec1_ddim = [&](auto g) { return dec1_launch<EPI_DDIM, decltype(g)::value>(a, dt, st); };
    if (layer == 8) {
        LDM_REQUIRE(ksv != 3 || (win && a.Wq % 64 == 0), "dec1 (variant 3): 64-column rows");
        geo = dec1_geo(ksv, W, a.Wq);
        if (s.keep_base) return step_dec1_keep(geo, a, s, st);
        if (s.plain || s.guide_eb) return step_dec1_guided(geo, a, s, st);
        LDM_REQUIRE(s.xs && s.coef, "dec1: sampler state, coefficients");
    }
    if (ksv == 3) {
        switch (layer) {
            case 0: LDM_REQUIRE(s.y && win && a.Wq % 64 == 0, "enc1 (variant 3): y, 64-column rows");
                return launch<0, 32, 64, 2, 1, 4, 2, 9, 9, EPI_RELU | EPI_WINDOW, 1>(a, dt, st);
            case 1: LDM_REQUIRE(s.y && s.bcast && win && a.Wq % 32 == 0, "enc2 (variant 3): y, t_emb, 32-column rows");
                return launch<1, 64, 128, 2, 1, 2, 4, 9, 9, EPI_RELU | EPI_BCAST | EPI_WINDOW, 1>(a, dt, st);
            case 2: LDM_REQUIRE(s.y && win && a.Wq % 16 == 0, "enc3 (variant 3): y, 16-column rows");
                return launch<1, 128, 256, 2, 1, 1, 8, 9, 9, EPI_RELU | EPI_WINDOW, 1>(a, dt, st);
            case 6: LDM_REQUIRE(s.y && s.skip && win && a.Wq % 16 == 0, "dec3 (variant 3): y, skip, 16-column rows");
                return launch<2, 256, 128, 1, 1, 1, 16, 9, 9, EPI_RELU | EPI_SKIP | EPI_WINDOW, 1>(a, dt, st);
            case 7: LDM_REQUIRE(s.y && s.skip && win && a.Wq % 32 == 0, "dec2 (variant 3): y, skip, 32-column rows");
                return launch<2, 128, 64, 1, 2, 1, 8, 9, 9, EPI_RELU | EPI_SKIP | EPI_WINDOW, 1>(a, dt, st);
            case 8: return s.msolver ? dec1_ms(std::integral_constant<int, 0>{}) : dec1_ddim(std::integral_constant<int, 0>{});
            case 3: LDM_REQUIRE(s.y && pl416, "enc4 (variant 3): y, 4 x 16 input plane");
                return launch<1, 256, 512, 1, 1, 1, 16, 9, 9, EPI_RELU | EPI_POSB | EPI_PLANE, 1>(a, dt, st);
            case 5: LDM_REQUIRE(s.y && s.skip && pl28, "dec4 (variant 3): y, skip, 2 x 8 plane");
                if (dec4_par())   // no partial tiles: the workspace stays untouched
                    return launch<2, 512, 256, 1, 1, 1, 16, 10, 10, EPI_RELU | EPI_SKIP | EPI_PLANE, kTapClass>(a, dt, st);
                return launch<2, 512, 256, 1, 1, 1, 16, 9, 9, EPI_RELU | EPI_SKIP | EPI_PLANE, 2>(a, dt, st, k);
            default: return fail(2, "step conv: no K-split variant 3 for this layer");
        }
    }
    if (ksv == 2) {
        switch (layer) {
            case 3: LDM_REQUIRE(s.y, "enc4: y");
                return launch_opt<EPI_PLANE, 1, 256, 512, 1, 2, 1, 8, 9, 9, EPI_RELU | EPI_POSB, 2>(pl416, a, dt, st, k);
            case 4: LDM_REQUIRE(s.y, "bottleneck: y");
                return launch_opt<EPI_PLANE, 0, 512, 512, 1, 2, 2, 4, 18, 18, EPI_RELU | EPI_POSB, 4>(pl28, a, dt, st, k);
            case 5: LDM_REQUIRE(s.y && s.skip, "dec4: y, skip");
                return launch_opt<EPI_PLANE, 2, 512, 256, 1, 2, 1, 8, 9, 9, EPI_RELU | EPI_SKIP, 4>(pl28, a, dt, st, k);
            default: return fail(2, "step conv: no K-split variant 2 for this layer");
        }
    }
    if (ksv) {
        switch (layer) {
            case 2: LDM_REQUIRE(s.y, "enc3: y"); return launch<1, 128, 256, 2, 2, 1, 4, 9, 9, EPI_RELU, 2>(a, dt, st, k);
            case 3: LDM_REQUIRE(s.y, "enc4: y");   // (the canonical latent: a 2 x 8 output plane)
                return launch_opt<EPI_PLANE, 1, 256, 512, 2, 2, 1, 4, 9, 9, EPI_RELU | EPI_POSB, 4>(pl416, a, dt, st, k);
            case 4: LDM_REQUIRE(s.y, "bottleneck: y");   // (the canonical latent: one sample per lane group)
                return launch_opt<EPI_PLANE, 0, 512, 512, 2, 2, 1, 8, 9, 9, EPI_RELU | EPI_POSB, 4>(pl28, a, dt, st, k);
            case 5: LDM_REQUIRE(s.y && s.skip, "dec4: y, skip");
                return launch_opt<EPI_PLANE, 2, 512, 256, 2, 2, 1, 4, 9, 9, EPI_RELU | EPI_SKIP, 8>(pl28, a, dt, st, k);
            case 6: LDM_REQUIRE(s.y && s.skip, "dec3: y, skip");
                return launch<2, 256, 128, 2, 2, 1, 4, 9, 9, EPI_RELU | EPI_SKIP, 4>(a, dt, st, k);
            default: return fail(2, "step conv: no K-split variant for this layer");
        }
    }
    // the single-block forms; EPI_WINDOW where a block's columns lie in one row of the column grid
    switch (layer) {
        case 0: LDM_REQUIRE(s.y, "enc1: y");
            return launch_opt<EPI_WINDOW, 0, 32, 64, 2, 1, 4, 1, 18, 18, EPI_RELU>(win && a.Wq % 64 == 0, a, dt, st);
        case 1: LDM_REQUIRE(s.y && s.bcast, "enc2: y, t_emb");
            if (enc2_wide(W)) return launch_opt<EPI_WINDOW, 1, 64, 128, 1, 1, 4, 1, 36, 36, EPI_RELU | EPI_BCAST>(win, a, dt, st);
            return launch_opt<EPI_WINDOW, 1, 64, 128, 2, 2, 1, 4, 9, 9, EPI_RELU | EPI_BCAST>(win && a.Wq % 32 == 0, a, dt, st);
        case 2: LDM_REQUIRE(s.y, "enc3: y");
            if (enc3_thin(W)) return launch_opt<EPI_WINDOW, 1, 128, 256, 1, 1, 2, 2, 36, 36, EPI_RELU>(win, a, dt, st);
            return launch_opt<EPI_WINDOW, 1, 128, 256, 2, 1, 1, 4, 18, 18, EPI_RELU>(win && a.Wq % 16 == 0, a, dt, st);
        case 3: LDM_REQUIRE(s.y, "enc4: y"); return launch<1, 256, 512, 1, 1, 1, 4, 36, 36, EPI_RELU | EPI_POSB>(a, dt, st);
        case 4: LDM_REQUIRE(s.y, "bottleneck: y"); return launch<0, 512, 512, 1, 1, 1, 8, 36, 12, EPI_RELU | EPI_POSB>(a, dt, st);
        case 5: LDM_REQUIRE(s.y && s.skip, "dec4: y, skip");
            return launch<2, 512, 256, 1, 1, 1, 8, 36, 12, EPI_RELU | EPI_SKIP>(a, dt, st);
        case 6: LDM_REQUIRE(s.y && s.skip, "dec3: y, skip");
            return launch_opt<EPI_WINDOW, 2, 256, 128, 1, 1, 1, 4, 36, 36, EPI_RELU | EPI_SKIP>(win && a.Wq % 16 == 0, a, dt, st);
        case 7: LDM_REQUIRE(s.y && s.skip, "dec2: y, skip");
            return launch_opt<EPI_WINDOW, 2, 128, 64, 1, 2, 1, 4, 18, 18, EPI_RELU | EPI_SKIP>(win && a.Wq % 32 == 0, a, dt, st);
        default: return s.msolver ? dec1_visit(geo, dec1_ms) : dec1_visit(geo, dec1_ddim);
    }
}

int step_layout(const float* x, float* y, int B, int C, int HW, bool to_nhwc, hipStream_t st) {
    const int64_t n = (int64_t)B * C * HW;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    if (to_nhwc)
        hipLaunchKernelGGL(uc::nchw_to_nhwc_kernel, dim3(blocks), dim3(256), 0, st, x, y, C, HW, n);
    else
        hipLaunchKernelGGL(uc::nhwc_to_nchw_kernel, dim3(blocks), dim3(256), 0, st, x, y, C, HW, n);
    LDM_CHECK_LAUNCH("layout transpose");
    return 0;
}

}  // namespace ldm

using namespace ldm;

extern "C" int64_t ldm_step_packed_floats(int32_t layer) { return step_packed_floats(layer); }

#if (UCONV_DIAG & 4)
extern "C" int ldm_debug_uconv_stamps(unsigned long long* host, int nblocks) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(uc::g_uconv_stamps), sizeof(unsigned long long) * 5 * nblocks, 0,
                                    hipMemcpyDeviceToHost);
}
#endif

extern "C" int ldm_step_pack_weight_dt(int32_t layer, int32_t dtype, const float* w, float* packed, void* stream) {
    LDM_REQUIRE(layer >= 0 && layer <= 8 && w && packed, "step pack: bad argument");
    LDM_REQUIRE(dtype >= LDM_DT_F32 && dtype <= LDM_DT_BF16, "step pack: unknown operand precision");
    const uc::LayerGeo& g = uc::kGeo[layer];
    const int64_t total = step_packed_floats(layer);
    const dim3 grid((unsigned)((total + 255) / 256));
    const int tr = g.mode == 2 ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == LDM_DT_F32)
        hipLaunchKernelGGL(uc::uconv_pack_kernel<0>, grid, dim3(256), 0, st, w, packed, g.cin, g.cout, tr);
    else if (dtype == LDM_DT_F16)
        hipLaunchKernelGGL(uc::uconv_pack_kernel<LDM_DT_F16>, grid, dim3(256), 0, st, w, packed, g.cin, g.cout, tr);
    else
        hipLaunchKernelGGL(uc::uconv_pack_kernel<LDM_DT_BF16>, grid, dim3(256), 0, st, w, packed, g.cin, g.cout, tr);
    LDM_CHECK_LAUNCH("uconv_pack_kernel");
    return 0;
}

extern "C" int ldm_step_pack_weight(int32_t layer, const float* w, float* packed, void* stream) {
    return ldm_step_pack_weight_dt(layer, LDM_DT_F32, w, packed, stream);
}

extern "C" int ldm_step_conv(int32_t layer, int32_t B, int32_t H, int32_t W, const float* x, const float* packed,
                             const float* bias, const float* bcast, const float* skip, float* y, void* stream) {
    return ldm_step_conv_dt(layer, B, H, W, x, packed, bias, bcast, skip, y, LDM_DT_F32, stream);
}

extern "C" int64_t ldm_step_workspace_floats(int32_t B, int32_t H, int32_t W) {
    if (B <= 0 || H % 8 || W % 8) return -1;
    return step_ws_floats(B, H, W, nullptr);
}

extern "C" int64_t ldm_step_workspace_counter_floats(int32_t B, int32_t H, int32_t W) {
    if (B <= 0 || H % 8 || W % 8) return -1;
    int64_t c = 0;
    step_ws_floats(B, H, W, &c);
    return c;
}

extern "C" int ldm_step_conv_ws(int32_t layer, int32_t B, int32_t H, int32_t W, const float* x, const float* packed,
                                const float* bias, const float* bcast, const float* skip, float* y, int32_t dtype,
                                float* workspace, void* stream) {
    StepConv s{};
    s.dtype = dtype;
    s.x = x;
    s.w = packed;
    s.bias = bias;
    s.bcast = bcast;
    s.skip = skip;
    s.y = y;
    s.ws = workspace;
    LDM_REQUIRE(layer != 8, "ldm_step_conv: dec1 runs fused with the DDIM update (ldm_sample)");
    return step_conv(layer, B, H, W, s, (hipStream_t)stream);
}

// (without a workspace every layer runs its single-block form)
extern "C" int ldm_step_conv_dt(int32_t layer, int32_t B, int32_t H, int32_t W, const float* x, const float* packed,
                                const float* bias, const float* bcast, const float* skip, float* y, int32_t dtype,
                                void* stream) {
    return ldm_step_conv_ws(layer, B, H, W, x, packed, bias, bcast, skip, y, dtype, nullptr, stream);
}

extern "C" int ldm_step_dec1_ddim(int32_t B, int32_t H, int32_t W, const float* d2, const float* packed, const float* bias,
                                  const float* coef, float eta, float* xs, float* x0_log, float* eps_log, int32_t dtype,
                                  void* stream) {
    LDM_REQUIRE(d2 && packed && bias && coef && xs, "ldm_step_dec1_ddim: null argument");
    StepConv s{};
    s.dtype = dtype;
    s.x = d2;
    s.w = packed;
    s.bias = bias;
    s.coef = coef;
    s.eta = eta;
    s.xs = xs;
    s.x0_log = x0_log;
    s.eps_log = eps_log;
    return step_conv(8, B, H, W, s, (hipStream_t)stream);
}

extern "C" int ldm_step_dec1_msolver(int32_t B, int32_t H, int32_t W, const float* d2, const float* packed,
                                     const float* bias, const float* coef, float* xs, const float* x0_prev, float* x0_log,
                                     float* eps_log, int32_t dtype, void* stream) {
    LDM_REQUIRE(d2 && packed && bias && coef && xs && x0_log, "ldm_step_dec1_msolver: null argument");
    LDM_REQUIRE(x0_prev != x0_log, "ldm_step_dec1_msolver: x0_prev must not be the x0 output");
    StepConv s{};
    s.dtype = dtype;
    s.x = d2;
    s.w = packed;
    s.bias = bias;
    s.coef = coef;
    s.xs = xs;
    s.msolver = 1;
    s.x0_prev = x0_prev;
    s.x0_log = x0_log;
    s.eps_log = eps_log;
    return step_conv(8, B, H, W, s, (hipStream_t)stream);
}
