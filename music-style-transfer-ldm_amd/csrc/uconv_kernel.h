// The step kernel of the reverse loop and its launchers: what uconv.hip (the unguided instances and the host side),
// uconv_guide.hip and uconv_keep.hip (dec1's guided / regional-keep instances, a code object each) share.  The design
// is described at the top of uconv.hip.
#pragma once
#include <algorithm>
#include <type_traits>
#include <utility>

#include "common.h"

#pragma clang fp contract(off)

namespace ldm {
namespace uc {

enum : int { EPI_RELU = 1, EPI_BCAST = 2, EPI_SKIP = 4, EPI_POSB = 8, EPI_DDIM = 16, EPI_PLANE = 32, EPI_WINDOW = 64, EPI_MSOLVER = 128, EPI_GUIDE = 256, EPI_KEEP = 512 };
// EPI_MSOLVER: dec1's epilogue is the multistep solver's update (msolver_update) in place of EPI_DDIM's; its
// instances are separate ones, so the EPI_DDIM instances are compiled exactly as without it.
// EPI_GUIDE (with EPI_DDIM or EPI_MSOLVER, again as separate instances): dec1 of the guided loop's target half.  The
// launch covers the caller's B samples; the base half's noise prediction e_b (written just before by the same
// geometry as a plain conv, NHWC) and the sample's strength are prefetched with the other epilogue operands, the
// output becomes guide_eps(o, e_b, s) before the update, and the new state is stored to both halves' copies.
// EPI_KEEP (with EPI_DDIM or EPI_MSOLVER, with or without EPI_GUIDE, separate instances once more): the regional keep.
// The update's result is blended with the content's own noising trajectory (keep_blend) before it is stored; z0, n0,
// the pixel's keep weight and the step's (a, b) are prefetched with the other epilogue operands.  The logs stay the
// model's own prediction.
// EPI_PLANE (a geometry flag carried with the epilogue bits): the layer's plane is 2 x 8 (the bottleneck at the
// canonical 16 x 64 latent), so the 16 columns of a lane group are one sample's whole plane and every tap of a
// stride-1 3x3 conv reads a position some lane of the group already holds.  Each channel chunk's activation
// fragment is loaded once (the centre tap), parked in the wave's own LDS window, and the other eight taps are
// read back shifted by 8 dy + dx positions (zero outside the plane): 1 global load per channel chunk instead of
// 9.  The stride-2 layer onto that plane (enc4, input 4 x 16) parks each sample's whole input plane instead:
// 4 loads instead of 9.  Needs MODE 0 / 1, a single stage, whole channel chunks per stage.
// EPI_WINDOW (likewise a geometry flag): a layer whose wave covers 16 TN consecutive columns of ONE row of its
// column grid (Wq a multiple of the block's columns): the wave loads the input rows and columns those columns'
// taps read (stride 1: 3 x (16 TN + 2); stride 2: 3 x (32 TN + 1); transposed: 2 x (16 TN + 1); halo and
// padding included, zeros outside the image) once per channel chunk, parks them in LDS and reads every tap from
// there: ceil(positions / 16) global loads per channel chunk instead of 9 TN (4 TN transposed).

struct UArgs {
    const float* x;       // NHWC [B, Hin, Win, CIN]
    const float* w;       // packed [9*CIN/16][COUT][16]
    float* y;             // NHWC [B, Hout, Wout, COUT] (unused with EPI_DDIM)
    const float* bias;    // [COUT], or with EPI_POSB [Hout*Wout][COUT]
    const float* bcast;   // [B][COUT]
    const float* skip;    // NHWC like y
    const float* coef;    // EPI_DDIM: [4] {sqrt(ab_t), sqrt(1-ab_t), sqrt(ab_n), sqrt(1-ab_n)}
    float* xs;            // EPI_DDIM: sampler state x, NHWC, updated in place
    float* x0_log;        // EPI_DDIM: pred_x0 log, NCHW [B, COUT, Hout, Wout] (or NULL)
    float* eps_log;       // EPI_DDIM: noise_pred log, NCHW (or NULL)
    float eta;
    int32_t B, Hin, Win, Hout, Wout;
    int32_t Hq, Wq, Nq;   // column grid: output pixels (conv) or input pixels (transposed)
    int32_t nMt, nNt, order;
    int32_t xpm, xpn;     // order 2: the 8 XCDs as an xpm x xpn grid over (M tiles, N tiles), contiguous slices
    FastDiv fd_hw, fd_w, fd_mt, fd_nt, fd_tiles;
    float* slab;          // KS > 1: partial tiles [tile][KS][NFR][64] float4 (write-through)
    int32_t* cnt;         // KS > 1: arrival counter per tile (zero between launches)
    const float* x0_prev; // EPI_MSOLVER: the previous step's pred_x0 log (NCHW like x0_log), or NULL (first-order step);
                          // coef is then the [8] row {alpha_t, sigma_t, c_x, c_0, c_1, ...} and x0_log is required
    // EPI_GUIDE adds no field (the kernarg block of every step launch stays the size it was): it reads the base half's
    // noise prediction (NHWC like xs) from `skip`, the guidance strength per sample [B] from `bcast`, and stores the
    // base half's copy of the sampler state through `y`: the three slots dec1's fused update leaves unused
    // EPI_KEEP adds none either.  `skip` is the loop's keep region [z0 | n0 | w] (z0 / n0 NHWC like xs, w [B, H, W])
    // and `bcast` the step's row {a, b}; with EPI_GUIDE the region is [e_b | z0 | n0 | w] and the row
    // {a, b, scale[B]}, so e_b is still read from `skip` and the strengths from `bcast`, two floats further on
};

// What a launch's head reads before its first operand load, passed as plain leading kernel parameters in front of
// UArgs (13 dwords): gfx950 delivers leading scalar parameters in SGPRs at wave launch (kernarg preload, enabled per
// translation unit in the Makefile), so the descriptors, the tile decode and the column arithmetic start without
// waiting for the kernarg segment's cold scalar load.  A by-value struct is not preloaded, hence plain parameters;
// UArgs keeps what the epilogue and the general decode read.  make_head fills it from the finished UArgs.
struct UHead {
    const float* w;       // = UArgs::w
    const float* x;       // = UArgs::x
    int32_t xbytes;       // bytes of x (the activation buffer descriptor's range)
    uint32_t dec;         // block order in bits 0-1; order 2: log2 xpn in bits 2-3, log2(nMt / xpm) in bits 4-7,
                          // nNt / xpn in bits 8-31 (set_grid takes order 2 only where these are exact)
    int32_t tiles;        // nMt * nNt
    int32_t Nq, Hin, Win;
    uint32_t mul_hw, mul_w;   // FastDiv::mul of fd_hw / fd_w
    uint32_t shr;         // fd_hw: shr in bits 0-4, `one` in bit 5; fd_w: the same in bits 8-12, 13
    __device__ __forceinline__ int div_hw(int n) const {
        return (int)((__umulhi((uint32_t)n, mul_hw) >> (shr & 31u)) + ((uint32_t)n & (0u - ((shr >> 5) & 1u))));
    }
    __device__ __forceinline__ int div_w(int n) const {
        return (int)((__umulhi((uint32_t)n, mul_w) >> ((shr >> 8) & 31u)) + ((uint32_t)n & (0u - ((shr >> 13) & 1u))));
    }
};

// (ky, kx) of tap t and the conv input offset / the transposed conv's output parity
__host__ __device__ constexpr int tky(int t) { return t / 3; }
__host__ __device__ constexpr int tkx(int t) { return t % 3; }
__host__ __device__ constexpr int tphase(int t) { return (tky(t) != 1 ? 2 : 0) + (tkx(t) != 1 ? 1 : 0); }
// The transposed layers read only four distinct input offsets over their nine taps (tap (ky, kx) reads input
// (qy + [ky == 0], qx + [kx == 0])): the activation fragment of a tap is loaded once per (channel chunk,
// offset) within a stage and reused by the other taps with that offset.  B_SRC<MODE, S>(i): the chunk of the
// stage whose fragment chunk i uses (i itself when it loads).
__host__ __device__ constexpr int toff(int t) { return (tky(t) == 0 ? 2 : 0) + (tkx(t) == 0 ? 1 : 0); }
// Tap classes of the transposed layers (TC; 0: all nine taps).  Each tap feeds one output parity, so the taps split
// into two classes with disjoint outputs: class 1 = the four taps of parity (odd, odd) (ky, kx in {0, 2}), class 2 =
// the other five, which cover parities (even, even), (even, odd) and (odd, even) = tphase 0, 1, 2.  A block that
// carries one class over ALL input channels finishes its parities by itself: no partial tile leaves the block.
constexpr int kTapClass = -1;   // value of the kernels' KS slot: blocks = tiles x the two tap classes
__host__ __device__ constexpr int tc_ntap(int TC) { return TC == 1 ? 4 : (TC == 2 ? 5 : 9); }
__host__ __device__ constexpr int tc_tap(int TC, int i) {
    return TC == 1 ? 6 * (i >> 1) + 2 * (i & 1) : (TC == 2 ? (i == 0 ? 1 : (i == 4 ? 7 : i + 2)) : i);
}
__host__ __device__ constexpr int tc_nph(int MODE, int TC) { return MODE != 2 ? 1 : (TC == 1 ? 1 : (TC == 2 ? 3 : 4)); }
template <int MODE, int TC = 0>
__host__ __device__ constexpr int b_src(int st, int S, int i) {
    if (MODE != 2) return i;
    constexpr int CPC = tc_ntap(TC);
    const int c = st * S + i;
    for (int j = 0; j < i; ++j) {
        const int cj = st * S + j;
        if (cj / CPC == c / CPC && toff(tc_tap(TC, cj % CPC)) == toff(tc_tap(TC, c % CPC))) return j;
    }
    return i;
}
// the first chunk of a channel chunk's taps that reads offset (0, 0), the lane's own position
__host__ __device__ constexpr int tc_own(int TC) {
    for (int i = 0; i < tc_ntap(TC); ++i)
        if (toff(tc_tap(TC, i)) == 0) return i;
    return -1;
}

// Diagnostic builds only (never shipped; tools/step_diag.sh): UCONV_DIAG bit 0 = no MFMAs, bit 1 = no
// operand loads, bit 2 = per-block timestamps of wave 0 (entry and exit in 100 MHz wall ticks, the
// phases between in shader clocks) into g_uconv_stamps, read back with ldm_debug_uconv_stamps.
#ifndef UCONV_DIAG
#define UCONV_DIAG 0
#endif
// cache policy of the activation (B operand) loads: 0 default; experiment builds set 2 (nt: streamed, so that
// they do not push the layer weights out of the XCD's L2 between iterations)
#ifndef UCONV_XAUX
#define UCONV_XAUX 0
#endif
#if (UCONV_DIAG & 4)
__device__ unsigned long long g_uconv_stamps[4096][5];
#define UCONV_STAMP(k)                                                                                 \
    do {                                                                                               \
        if (threadIdx.x == 0 && blockIdx.x < 4096u)                                                    \
            g_uconv_stamps[blockIdx.x][k] = ((k) == 0 || (k) == 4) ? __builtin_amdgcn_s_memrealtime() \
                                                                   : __builtin_amdgcn_s_memtime();    \
    } while (0)
#else
#define UCONV_STAMP(k) \
    do {               \
    } while (0)
#endif

// compile-time loop: f(integral_constant<int, I>) for I in [B, E)
template <int B, int E, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        static_for<B + 1, E>(f);
    }
}

template <int MODE, int CIN, int COUT, int TM, int TN, int WN, int WK, int NCH, int S, int EPI, int DT, int KS, int TC = 0>
__device__ __forceinline__ void uconv_body(const UHead& h, const UArgs& a, int bid_in) {
    constexpr int NPH = tc_nph(MODE, TC);         // accumulator sets: the output parities this block finishes
    constexpr int NST = NCH / S;
    constexpr int CPC = tc_ntap(TC);              // chunks per channel chunk (the 9 taps, or the taps of class TC)
    static_assert(NCH % S == 0 && NCH % CPC == 0, "stage / chunk structure");
    static_assert(CIN % 16 == 0 && COUT % (16 * TM) == 0, "channel tiling");
    static_assert(CIN / 16 == (NCH / CPC) * WK * KS, "the grid's waves cover K exactly once");
    static_assert(TC == 0 || (MODE == 2 && KS == 1 && (EPI & EPI_PLANE) != 0), "tap classes: transposed plane form");
    // a lone accumulator chain of 16x16x4 (40-cycle dependent latency, 32-cycle issue) alternates two
    constexpr int NACC2 = (NPH * TM * TN == 1) ? 2 : 1;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    UCONV_STAMP(0);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wn = wave % WN, wk = wave / WN;
    const int col = lane & 15, lg = lane >> 4;

    // block -> (K split ks, M tile, N tile).  The KS blocks of one tile are tiles apart, so with a tile count
    // that is a multiple of 8 they share an XCD (round-robin placement): the last one reads the others'
    // partials from its own L2.
    int mt, nt, ks = 0;
    {
        int bid = bid_in;
        if constexpr (KS > 1) {
            ks = a.fd_tiles.div(bid);
            bid -= ks * h.tiles;
        }
        if ((h.dec & 3u) == 2u) {
            // XCD-aware: tile T goes to XCD T % 8 (round-robin placement); XCD x = (xm, xn) owns the contiguous
            // M-tile slice xm and N-tile slice xn, so it fetches 1/xpm of the weights and 1/xpn of the input
            // (and the input rows a slice shares with its neighbour once).  xpn and the M tiles per slice are
            // powers of two (set_grid): the decode is shifts and masks of the preloaded record
            const int spn = (h.dec >> 2) & 3u, sml = (h.dec >> 4) & 15u, nloc = (int)(h.dec >> 8);
            const int x = bid & 7, l = bid >> 3;
            const int xm = x >> spn, xn = x & ((1 << spn) - 1);
            const int ln = l >> sml;
            mt = (xm << sml) + (l & ((1 << sml) - 1));
            nt = xn * nloc + ln;
        } else {
            const int q1 = a.fd_mt.div(bid), q2 = a.fd_nt.div(bid);
            mt = a.order == 0 ? bid - q1 * a.nMt : q2;
            nt = a.order == 0 ? q1 : bid - q2 * a.nNt;
        }
    }
    const int m0 = mt * (16 * TM);
    const int nbase = nt * (16 * TN * WN) + wn * (16 * TN);

    // per column: (b, qy, qx) and the per-tap input byte offsets (kOOB: padding / outside the image)
    constexpr int kOOB = 0x7ffffff0;
    int vt[9][TN];
    int cb[TN], cqy[TN], cqx[TN];
    bool cval[TN];
    // (the column grid from the preloaded input plane: output pixels of a conv, input pixels of a transposed one)
    const int Hin = h.Hin, Win = h.Win;
    const int Hq = MODE == 1 ? Hin / 2 : Hin, Wq = MODE == 1 ? Win / 2 : Win;
#pragma unroll
    for (int ni = 0; ni < TN; ++ni) {
        const int n = nbase + 16 * ni + col;
        const bool nv = n < h.Nq;
        const int nn = nv ? n : 0;
        const int b = h.div_hw(nn);
        const int r = nn - b * (Hq * Wq);
        const int qy = h.div_w(r);
        const int qx = r - qy * Wq;
        cb[ni] = b;
        cqy[ni] = qy;
        cqx[ni] = qx;
        cval[ni] = nv;
        const int iy0 = MODE == 0 ? qy - 1 : (MODE == 1 ? 2 * qy - 1 : qy);
        const int ix0 = MODE == 0 ? qx - 1 : (MODE == 1 ? 2 * qx - 1 : qx);
        const int base = ((b * Hin + iy0) * Win + ix0) * (CIN * 4) + lg * 16;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int ky = tky(t), kx = tkx(t);
            const int dy = MODE == 2 ? (ky == 0 ? 1 : 0) : ky;
            const int dx = MODE == 2 ? (kx == 0 ? 1 : 0) : kx;
            const bool ok = nv && (unsigned)(iy0 + dy) < (unsigned)Hin && (unsigned)(ix0 + dx) < (unsigned)Win;
            vt[t][ni] = ok ? base + (dy * Win + dx) * (CIN * 4) : kOOB;
        }
    }

    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
        uni_ptr(h.x), (short)0, uni(h.xbytes), 0x00020000);
    // 16-bit operands read 16-bit packed weights (ldm_step_pack_weight_dt): half the A bytes of the fp32 pack,
    // which matters because a block's operand stream through its CU's L1 is what bounds these launches
    constexpr int AE = DT != 0 ? 2 : 4;                        // bytes per packed weight element
    using AT = std::conditional_t<DT != 0, shortx4, floatx4>;
    constexpr int WBYTES = 9 * CIN * COUT * AE;
    const __amdgpu_buffer_rsrc_t wr =
        __builtin_amdgcn_make_buffer_rsrc(uni_ptr(h.w), (short)0, WBYTES, 0x00020000);
    const int va = ((m0 + col) * 16 + lg * 4) * AE;            // A: row m0+col, k-local 4*lg .. +3
    const int kw0 = ks * WK + wk;                              // this wave's slice of K
    const int sa0 = uni(kw0 * (NCH / CPC) * 9 * COUT * 16 * AE);   // first chunk (tap 0) of its first channel chunk
    const int sb0 = uni(kw0 * (NCH / CPC) * 64);               // its first channel chunk (16 ch x 4 B)

    floatx4 acc[NACC2][NPH][TM][TN];
#pragma unroll
    for (int u = 0; u < NACC2; ++u)
#pragma unroll
        for (int p = 0; p < NPH; ++p)
#pragma unroll
            for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                for (int ni = 0; ni < TN; ++ni) acc[u][p][mi][ni] = floatx4{0.f, 0.f, 0.f, 0.f};

    constexpr int XAUX = UCONV_XAUX;
    AT fa[NST > 1 ? 2 : 1][S][TM];
    floatx4 fb[NST > 1 ? 2 : 1][S][TN];
    // PART bit 0: weight (A) fragments, bit 1: activation (B) fragments
    auto load_stage = [&](auto stc, auto partc) {
        constexpr int st = decltype(stc)::value;
        constexpr int PART = decltype(partc)::value;
        constexpr int bf = NST > 1 ? (st & 1) : 0;
        static_for<0, S>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            constexpr int c = st * S + i;                 // chunk within this wave's range
            constexpr int t = tc_tap(TC, c % CPC), cc = c / CPC;
            constexpr int cw = cc * 9 + t;                // ... and within the wave's packed weights
            if constexpr ((PART & 1) != 0)
#pragma unroll
            for (int mi = 0; mi < TM; ++mi) {
                const int so = sa0 + (cw * COUT * 16 + mi * 256) * AE;
                if constexpr ((UCONV_DIAG & 2) != 0)
                    fa[bf][i][mi] = AT{};
                else if constexpr (DT != 0)
                    fa[bf][i][mi] = __builtin_bit_cast(shortx4, __builtin_amdgcn_raw_buffer_load_b64(wr, va, so, 0));
                else
                    fa[bf][i][mi] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(wr, va, so, 0));
            }
            if constexpr ((PART & 2) != 0 && b_src<MODE, TC>(st, S, i) == i)
#pragma unroll
            for (int ni = 0; ni < TN; ++ni)
                fb[bf][i][ni] = (UCONV_DIAG & 2) ? floatx4{(float)vt[t][ni], 1.f, 2.f, 3.f}
                                                 : __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(
                                                                                   xr, vt[t][ni], sb0 + cc * 64, XAUX));
            __builtin_amdgcn_sched_barrier(0);        // chunks issue in consumption order
        });
    };
    auto compute_stage = [&](auto stc) {
        constexpr int st = decltype(stc)::value;
        constexpr int bf = NST > 1 ? (st & 1) : 0;
        static_for<0, S>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            constexpr int c = st * S + i;
            // (class 1 has the one parity 3 = set 0; class 2's parities are tphase 0..2, its sets in that order)
            constexpr int p = MODE == 2 && TC != 1 ? tphase(tc_tap(TC, c % CPC)) : 0;
            constexpr int ib = b_src<MODE, TC>(st, S, i);   // the fragment this chunk's taps share
            if constexpr (DT != 0) {   // fp16 / bf16 operands: the whole 16-channel chunk in one MFMA
                constexpr int u = NACC2 == 2 ? (c & 1) : 0;
#pragma unroll
                for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                    for (int ni = 0; ni < TN; ++ni)
                        acc[u][p][mi][ni] = mma16_lowp<DT>(fa[bf][i][mi], fb[bf][ib][ni], acc[u][p][mi][ni]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                        for (int ni = 0; ni < TN; ++ni) {
                            const int u = NACC2 == 2 ? (j & 1) : 0;
                            if constexpr ((UCONV_DIAG & 1) != 0) {   // diagnostic: no MFMAs (operands kept live)
                                if (j == 0)
                                    acc[u][p][mi][ni][0] = acc[u][p][mi][ni][0] + fa[bf][i][mi][j] * fb[bf][ib][ni][j];
                            } else {
                                acc[u][p][mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                                    fa[bf][i][mi][j], fb[bf][ib][ni][j], acc[u][p][mi][ni], 0, 0, 0);
                            }
                        }
            }
        });
    };
    // Epilogue operands of the fragments this thread finishes — fragment f = k*WK + wk for k < NMY (all
    // of them when WK == 1) — loaded right after the last operand stage is issued: they arrive while the
    // MFMAs run and never hold up an operand wait.  Branch-free (a fragment index past NFR is clamped
    // and its result dropped), so the waitcnt pass sees one straight-line load sequence.
    constexpr int NFR = NPH * TM * TN;   // accumulator fragments per wave
    constexpr int NMY = (NFR + WK - 1) / WK;
    static_assert(TN <= 2, "column selects below assume TN <= 2");
    auto frag = [&](int k) { return WK == 1 ? k : k * WK + wk; };
    // (a bitwise blend of two scalars: a ?: over array elements gets folded into a dynamically indexed
    // array, which lives in scratch memory)
    auto colsel = [&](const auto& arr, int ni) -> int {
        const int v0 = (int)arr[0], v1 = (int)arr[TN - 1];
        return TN == 1 ? v0 : (v0 ^ ((v0 ^ v1) & -(int)(ni != 0)));
    };
    struct Out {
        int b, oy, ox, pix, m;
        bool ok;
    };
    auto out_of = [&](int f) {
        const int fc = f < NFR ? f : NFR - 1;
        const int p = TC == 1 ? 3 : fc / (TM * TN), mi = (fc / TN) % TM, ni = fc % TN;   // p: the output parity
        Out o;
        o.b = colsel(cb, ni);
        o.oy = MODE == 2 ? 2 * colsel(cqy, ni) + (p >> 1) : colsel(cqy, ni);
        o.ox = MODE == 2 ? 2 * colsel(cqx, ni) + (p & 1) : colsel(cqx, ni);
        o.pix = (o.b * a.Hout + o.oy) * a.Wout + o.ox;
        o.m = m0 + 16 * mi + 4 * lg;
        o.ok = f < NFR && colsel(cval, ni) != 0;
        return o;
    };
    floatx4 pre_b[NMY], pre_c[NMY], pre_s[NMY], pre_h[NMY], pre_g[NMY], pre_kz[NMY], pre_kn[NMY];
    float pre_gs[NMY], pre_kw[NMY], pre_ka = 0.f, pre_kb = 0.f;
    constexpr int KROW = (EPI & EPI_KEEP) ? 2 : 0;   // the strengths' offset in `bcast`
    auto epi_prefetch = [&]() {
        static_for<0, NMY>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            const Out o = out_of(frag(k));
            pre_b[k] = (EPI & EPI_POSB)
                           ? *reinterpret_cast<const floatx4*>(a.bias + (size_t)(o.oy * a.Wout + o.ox) * COUT + o.m)
                           : *reinterpret_cast<const floatx4*>(a.bias + o.m);
            if constexpr ((EPI & EPI_BCAST) != 0) pre_c[k] = *reinterpret_cast<const floatx4*>(a.bcast + (size_t)o.b * COUT + o.m);
            if constexpr ((EPI & EPI_SKIP) != 0) pre_s[k] = *reinterpret_cast<const floatx4*>(a.skip + (size_t)o.pix * COUT + o.m);
            if constexpr ((EPI & EPI_DDIM) != 0) pre_s[k] = *reinterpret_cast<const floatx4*>(a.xs + (size_t)o.pix * COUT + o.m);
            if constexpr ((EPI & EPI_MSOLVER) != 0) {
                pre_s[k] = *reinterpret_cast<const floatx4*>(a.xs + (size_t)o.pix * COUT + o.m);
                if (a.x0_prev) {   // uniform: the solver's history, read with the stride its log was written with
                    const size_t hw = (size_t)a.Hout * a.Wout;
                    const size_t lbase = ((size_t)o.b * COUT + o.m) * hw + (size_t)o.oy * a.Wout + o.ox;
#pragma unroll
                    for (int r = 0; r < 4; ++r) pre_h[k][r] = a.x0_prev[lbase + r * hw];
                }
            }
            if constexpr ((EPI & EPI_GUIDE) != 0) {
                pre_g[k] = *reinterpret_cast<const floatx4*>(a.skip + (size_t)o.pix * COUT + o.m);
                pre_gs[k] = a.bcast[KROW + o.b];
            }
            if constexpr ((EPI & EPI_KEEP) != 0) {
                constexpr int G = (EPI & EPI_GUIDE) ? 1 : 0;   // e_b in front of the keep operands
                const size_t ne = (size_t)a.B * a.Hout * a.Wout * COUT;
                pre_kz[k] = *reinterpret_cast<const floatx4*>(a.skip + G * ne + (size_t)o.pix * COUT + o.m);
                pre_kn[k] = *reinterpret_cast<const floatx4*>(a.skip + (G + 1) * ne + (size_t)o.pix * COUT + o.m);
                pre_kw[k] = a.skip[(G + 2) * ne + (size_t)o.pix];
            }
        });
        if constexpr ((EPI & EPI_KEEP) != 0) pre_ka = a.bcast[0], pre_kb = a.bcast[1];
    };

    // scheduling fences keep each stage's loads ahead of the MFMAs that consume the previous stage (the
    // default scheduler would interleave them to save registers and expose one latency per chunk); the
    // waitcnt pass then waits progressively, chunk by chunk, in issue order
    UCONV_STAMP(1);
    using AB = std::integral_constant<int, 3>;
    constexpr bool PLANE = (EPI & EPI_PLANE) != 0;
    static_assert(!PLANE || (NST == 1 && S % CPC == 0), "EPI_PLANE geometry");
    if constexpr (PLANE && MODE == 1) {
        // stride 2 onto a 2 x 8 output plane: each sample's whole 4 x 16 input plane (64 positions, 4 loads per
        // lane per channel chunk) goes to the wave's LDS window; tap (ky, kx) of output (qy, qx) reads input
        // (2 qy - 1 + ky, 2 qx - 1 + kx), zero where that is -1 (the top / left padding; the bottom / right
        // never pass the plane)
        constexpr int NCC = S / CPC;
        floatx4 wl[NCC][TN][4];
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) {
            const int bs = colsel(cb, ni);   // this column set's sample (16 columns = one sample)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int e = k * 64 + lane, pos = e >> 2, g4 = e & 3;
                const int off = colsel(cval, ni) ? ((bs * 4 + (pos >> 4)) * 16 + (pos & 15)) * (CIN * 4) + g4 * 16 : kOOB;
                static_for<0, NCC>([&](auto ccc) {
                    constexpr int cc = decltype(ccc)::value;
                    wl[cc][ni][k] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(xr, off, sb0 + cc * 64, XAUX));
                });
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        load_stage(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
        epi_prefetch();
        __builtin_amdgcn_sched_barrier(0);
        constexpr int kRedFloats = WK > 1 ? WK * WN * NPH * TM * TN * 64 * 4 : 0;
        float* win = smem + kRedFloats + wave * (NCC * TN * 1024);
        static_for<0, NCC>([&](auto ccc) {
            constexpr int cc = decltype(ccc)::value;
#pragma unroll
            for (int ni = 0; ni < TN; ++ni)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    *reinterpret_cast<floatx4*>(win + (cc * TN + ni) * 1024 + (k * 64 + lane) * 4) = wl[cc][ni][k];
        });
        // the taps read what OTHER lanes of this wave wrote: the compiler, which reasons per lane, may otherwise
        // hoist a read above a write it cannot alias (and the LDS hand back the previous launch's window).  A
        // wave's LDS operations execute in order, so the wave only waits for its own writes: no block barrier.
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const int qy = col >> 3, qx = col & 7;
        static_for<0, NCC>([&](auto ccc) {
            constexpr int cc = decltype(ccc)::value;
            static_for<0, CPC>([&](auto tc) {
                constexpr int t = decltype(tc)::value;
                const int iy = 2 * qy - 1 + tky(t), ix = 2 * qx - 1 + tkx(t);
                const bool in = iy >= 0 && ix >= 0;
                const int o = in ? (iy * 16 + ix) * 16 + lg * 4 : 0;
#pragma unroll
                for (int ni = 0; ni < TN; ++ni) {
                    const floatx4 v = *reinterpret_cast<const floatx4*>(win + (cc * TN + ni) * 1024 + o);
                    fb[0][cc * CPC + t][ni] = in ? v : floatx4{0.f, 0.f, 0.f, 0.f};
                }
            });
        });
    } else if constexpr (PLANE && MODE == 2) {
        // transposed conv over a 2 x 8 input plane: the four offsets a tap reads, (qy + oy, qx + ox) with oy, ox in
        // {0, 1}, are all in the sample's own plane (zero past its last row / column): one load per channel chunk
        // (OWN: the slot of the first tap in the list that reads offset (0, 0))
        constexpr int NCC = S / CPC;
        constexpr int OWN = tc_own(TC);
        static_for<0, NCC>([&](auto ccc) {
            constexpr int cc = decltype(ccc)::value;
#pragma unroll
            for (int ni = 0; ni < TN; ++ni)   // tap 8 = (2, 2) reads offset (0, 0): the lane's own position
                fb[0][cc * CPC + OWN][ni] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(
                                                                            xr, vt[8][ni], sb0 + cc * 64, XAUX));
        });
        __builtin_amdgcn_sched_barrier(0);
        load_stage(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
        epi_prefetch();
        __builtin_amdgcn_sched_barrier(0);
        constexpr int kRedFloats = WK > 1 ? WK * WN * NPH * TM * TN * 64 * 4 : 0;
        float* win = smem + kRedFloats + wave * (NCC * TN * 256);
        const int py = col >> 3, px = col & 7;
        static_for<0, NCC>([&](auto ccc) {
            constexpr int cc = decltype(ccc)::value;
#pragma unroll
            for (int ni = 0; ni < TN; ++ni)
                *reinterpret_cast<floatx4*>(win + ((cc * TN + ni) * 16 + col) * 16 + lg * 4) = fb[0][cc * CPC + OWN][ni];
        });
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // cross-lane through LDS: see the stride-2 plane branch
        static_for<0, NCC>([&](auto ccc) {
            constexpr int cc = decltype(ccc)::value;
            static_for<0, CPC>([&](auto tc) {
                constexpr int t = tc_tap(TC, decltype(tc)::value);
                constexpr int i = cc * CPC + decltype(tc)::value;
                if constexpr (b_src<MODE, TC>(0, S, i) == i) {
                    constexpr int oy = tky(t) == 0 ? 1 : 0, ox = tkx(t) == 0 ? 1 : 0;
                    const bool in = py + oy < 2 && px + ox < 8;
#pragma unroll
                    for (int ni = 0; ni < TN; ++ni) {
                        const floatx4 v =
                            *reinterpret_cast<const floatx4*>(win + ((cc * TN + ni) * 16 + col + 8 * oy + ox) * 16 + lg * 4);
                        fb[0][i][ni] = in ? v : floatx4{0.f, 0.f, 0.f, 0.f};
                    }
                }
            });
        });
    } else if constexpr (PLANE) {
        constexpr int NCC = S / CPC;   // channel chunks of this wave
        // centre taps first (the window waits on them only), then the weight stream, then the epilogue operands
        static_for<0, NCC>([&](auto ccc) {
            constexpr int cc = decltype(ccc)::value;
#pragma unroll
            for (int ni = 0; ni < TN; ++ni)
                fb[0][cc * CPC + 4][ni] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(
                                                                          xr, vt[4][ni], sb0 + cc * 64, XAUX));
        });
        __builtin_amdgcn_sched_barrier(0);
        load_stage(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
        epi_prefetch();
        __builtin_amdgcn_sched_barrier(0);
        // the wave's window: [cc][ni][16 positions][16 channels] fp32, after the K-reduction buffer
        constexpr int kRedFloats = WK > 1 ? WK * WN * NPH * TM * TN * 64 * 4 : 0;
        float* win = smem + kRedFloats + wave * (NCC * TN * 256);
        const int py = col >> 3, px = col & 7;
        static_for<0, NCC>([&](auto ccc) {
            constexpr int cc = decltype(ccc)::value;
#pragma unroll
            for (int ni = 0; ni < TN; ++ni)
                *reinterpret_cast<floatx4*>(win + ((cc * TN + ni) * 16 + col) * 16 + lg * 4) = fb[0][cc * CPC + 4][ni];
        });
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // cross-lane through LDS: see the stride-2 plane branch
        static_for<0, NCC>([&](auto ccc) {
            constexpr int cc = decltype(ccc)::value;
            static_for<0, CPC>([&](auto tc) {
                constexpr int t = decltype(tc)::value;
                if constexpr (t != 4) {
                    constexpr int dy = tky(t) - 1, dx = tkx(t) - 1;
                    const bool in = (unsigned)(py + dy) < 2u && (unsigned)(px + dx) < 8u;
#pragma unroll
                    for (int ni = 0; ni < TN; ++ni) {
                        const floatx4 v =
                            *reinterpret_cast<const floatx4*>(win + ((cc * TN + ni) * 16 + col + 8 * dy + dx) * 16 + lg * 4);
                        fb[0][cc * CPC + t][ni] = in ? v : floatx4{0.f, 0.f, 0.f, 0.f};
                    }
                }
            });
        });
    } else if constexpr ((EPI & EPI_WINDOW) != 0) {
        static_assert(NST == 1 && S % CPC == 0, "EPI_WINDOW geometry");
        constexpr int NCC = S / CPC;           // channel chunks of this wave
        // the input rows and columns the wave's 16 TN output columns (one row of the column grid) read:
        // stride 1: rows y0-1..y0+1, columns x0-1..x0+16TN; stride 2: rows 2y0-1..2y0+1, columns
        // 2x0-1..2x0+32TN-1; transposed (input grid): rows y0..y0+1, columns x0..x0+16TN
        constexpr int WR = MODE == 2 ? 2 : 3;
        constexpr int WC = MODE == 0 ? 16 * TN + 2 : (MODE == 1 ? 32 * TN + 1 : 16 * TN + 1);
        constexpr int WPOS = WR * WC;          // window positions
        constexpr int NLD = (WPOS * 4 + 63) / 64;   // 16-byte loads per lane per channel chunk
        const int b0 = h.div_hw(nbase);
        const int rem = nbase - b0 * (Hq * Wq);
        const int y0 = h.div_w(rem);
        const int x0 = rem - y0 * Wq;
        const int iy0 = MODE == 0 ? y0 - 1 : (MODE == 1 ? 2 * y0 - 1 : y0);
        const int ix0 = MODE == 0 ? x0 - 1 : (MODE == 1 ? 2 * x0 - 1 : x0);
        floatx4 wl[NCC][NLD];
        int wpos[NLD];
        static_for<0, NLD>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            const int e = k * 64 + lane;       // window slot: (position, 4-channel group)
            const int pos = e >> 2, g4 = e & 3;
            const int r = pos / WC, cx = pos - r * WC;
            const int iy = iy0 + r, ix = ix0 + cx;
            const bool ok = e < WPOS * 4 && (unsigned)iy < (unsigned)Hin && (unsigned)ix < (unsigned)Win && nbase < h.Nq;
            const int off = ok ? ((b0 * Hin + iy) * Win + ix) * (CIN * 4) + g4 * 16 : kOOB;
            wpos[k] = e < WPOS * 4 ? pos * 16 + g4 * 4 : -1;
            static_for<0, NCC>([&](auto ccc) {
                constexpr int cc = decltype(ccc)::value;
                wl[cc][k] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(xr, off, sb0 + cc * 64, XAUX));
            });
        });
        __builtin_amdgcn_sched_barrier(0);
        load_stage(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
        epi_prefetch();
        __builtin_amdgcn_sched_barrier(0);
        constexpr int kRedFloats = WK > 1 ? WK * WN * NPH * TM * TN * 64 * 4 : 0;
        float* win = smem + kRedFloats + wave * (NCC * WPOS * 16);
        static_for<0, NLD>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            static_for<0, NCC>([&](auto ccc) {
                constexpr int cc = decltype(ccc)::value;
                if (wpos[k] >= 0) *reinterpret_cast<floatx4*>(win + cc * WPOS * 16 + wpos[k]) = wl[cc][k];
            });
        });
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // cross-lane through LDS: see the stride-2 plane branch
        static_for<0, NCC>([&](auto ccc) {
            constexpr int cc = decltype(ccc)::value;
            static_for<0, CPC>([&](auto tc) {
                constexpr int t = decltype(tc)::value;
                constexpr int i = cc * CPC + t;
                if constexpr (b_src<MODE>(0, S, i) == i) {   // transposed: one read per distinct offset
                    constexpr int wr = MODE == 2 ? (tky(t) == 0 ? 1 : 0) : tky(t);
                    constexpr int wx = MODE == 2 ? (tkx(t) == 0 ? 1 : 0) : tkx(t);
#pragma unroll
                    for (int ni = 0; ni < TN; ++ni) {
                        const int cx = MODE == 1 ? 2 * (16 * ni + col) + wx : 16 * ni + col + wx;
                        fb[0][i][ni] = *reinterpret_cast<const floatx4*>(win + cc * WPOS * 16 + (wr * WC + cx) * 16 + lg * 4);
                    }
                }
            });
        });
    } else {
        load_stage(std::integral_constant<int, 0>{}, AB{});
        if constexpr (NST == 1) epi_prefetch();
    }
    __builtin_amdgcn_sched_barrier(0);
    static_for<0, NST>([&](auto stc) {
        constexpr int st = decltype(stc)::value;
        if constexpr (st + 1 < NST) {
            load_stage(std::integral_constant<int, st + 1>{}, AB{});
            if constexpr (st + 2 == NST) epi_prefetch();
        }
        __builtin_amdgcn_sched_barrier(0);
        compute_stage(stc);
        __builtin_amdgcn_sched_barrier(0);
    });
    if constexpr (NACC2 == 2) {
#pragma unroll
        for (int p = 0; p < NPH; ++p)
#pragma unroll
            for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                for (int ni = 0; ni < TN; ++ni) acc[0][p][mi][ni] = acc[0][p][mi][ni] + acc[1][p][mi][ni];
    }

    UCONV_STAMP(2);
    // ---- in-block K reduction (fixed order) and the fused epilogue ------------------------------------
    floatx4* red = reinterpret_cast<floatx4*>(smem);
    if constexpr (WK > 1) {
        static_for<0, NFR>([&](auto fc) {
            constexpr int f = decltype(fc)::value;
            constexpr int p = f / (TM * TN), mi = (f / TN) % TM, ni = f % TN;
            red[((wk * WN + wn) * NFR + f) * 64 + lane] = acc[0][p][mi][ni];
        });
        __syncthreads();
    }
    UCONV_STAMP(3);
    floatx4 vv[NMY];
    static_for<0, NMY>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        const int f = frag(k);
        if constexpr (WK > 1) {
            const int fc = f < NFR ? f : NFR - 1;
            floatx4 v = red[((0 * WN + wn) * NFR + fc) * 64 + lane];
#pragma unroll
            for (int k2 = 1; k2 < WK; ++k2) v = v + red[((k2 * WN + wn) * NFR + fc) * 64 + lane];
            vv[k] = v;
        } else {
            constexpr int p = k / (TM * TN), mi = (k / TN) % TM, ni = k % TN;
            vv[k] = acc[0][p][mi][ni];
        }
    });
    if constexpr (KS > 1) {
        // ---- K split over blocks: write-through (sc1) partial tile, arrival counter, the last block of the
        //      tile sums the KS partials in split order (deterministic) and runs the epilogue ---------------
        const int tile = mt + nt * a.nMt;
        const __amdgpu_buffer_rsrc_t sr = __builtin_amdgcn_make_buffer_rsrc(uni_ptr(a.slab), (short)0, 0x7fffffff, 0x00020000);
        auto slab_off = [&](int kk, int f) { return ((((tile * KS + kk) * WN + wn) * NFR + f) * 64 + lane) * 16; };
        static_for<0, NMY>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            const int f = frag(k);
            if (f < NFR)
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, vv[k]),
                                                       sr, slab_off(ks, f), 0, 16);
        });
        // Ordering of the hand-off: the partial tile is stored write-through (sc1) and drained (vmcnt(0)) before
        // the block's barrier, and thread 0 counts the block only after that barrier; the last arriver reads the
        // other partials with sc1 loads after its own barrier, whose workgroup-scope acquire keeps the compiler
        // from hoisting them above the counter.  An agent-scope acq_rel RMW would order the same traffic through
        // the memory model, but on gfx950 it lowers to an L2 write-back + invalidate per block (the plain-store +
        // release form the guide's handoff-flag / publish-large rows price at 2-2.7x the sc1 form).
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        int* flag = reinterpret_cast<int*>(smem);
        if (threadIdx.x == 0) {
            const int old = __hip_atomic_fetch_add(a.cnt + tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int last = old == KS - 1;
            if (last) __hip_atomic_store(a.cnt + tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *flag = last;
        }
        __syncthreads();
        if (!*flag) return;
        static_for<0, NMY>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            const int f = frag(k);
            const int fc = f < NFR ? f : NFR - 1;
            floatx4 part[KS];
#pragma unroll
            for (int kk = 0; kk < KS; ++kk)
                part[kk] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(sr, slab_off(kk, fc), 0, 16));
            floatx4 sum = ks == 0 ? vv[k] : part[0];
#pragma unroll
            for (int kk = 1; kk < KS; ++kk) sum = sum + (kk == ks ? vv[k] : part[kk]);
            vv[k] = sum;
        });
    }
    static_for<0, NMY>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        const int f = frag(k);
        const floatx4 v = vv[k];
        const Out ot = out_of(f);
        if (!ot.ok) return;
        const floatx4 bias = pre_b[k];
        floatx4 o;
        // 16-bit operands (a sampling loop inside torch.autocast): the conv output and each add rounded to that
        // type as well, as the reference's autocast convs return 16-bit tensors; the DDIM update stays fp32
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float sv = round16(v[r] + bias[r], DT);
            if (EPI & EPI_RELU) sv = sv < 0.f ? 0.f : sv;
            o[r] = sv;
        }
        if constexpr ((EPI & EPI_BCAST) != 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = round16(o[r] + pre_c[k][r], DT);
        }
        if constexpr ((EPI & EPI_SKIP) != 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = round16(o[r] + pre_s[k][r], DT);
        }
        if constexpr ((EPI & EPI_GUIDE) != 0) {
            // o is the target half's noise prediction: guided against the base half's (guide_eps), fp32 whatever DT is
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = guide_eps(o[r], pre_g[k][r], pre_gs[k]);
        }
        if constexpr ((EPI & EPI_MSOLVER) != 0) {
            // noise_pred = o; the multistep update (msolver_update, one rounding per op), fp32 whatever DT is
            const floatx4 xv = pre_s[k];
            floatx4 xn;
            const bool hp = a.x0_prev != nullptr;
            const size_t hw = (size_t)a.Hout * a.Wout;
            const size_t lbase = ((size_t)ot.b * COUT + ot.m) * hw + (size_t)ot.oy * a.Wout + ot.ox;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float x0;
                xn[r] = msolver_update(xv[r], o[r], a.coef, hp, hp ? pre_h[k][r] : 0.f, x0);
                a.x0_log[lbase + r * hw] = x0;
                if (a.eps_log) a.eps_log[lbase + r * hw] = o[r];
            }
            if constexpr ((EPI & EPI_KEEP) != 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) xn[r] = keep_blend(xn[r], pre_kz[k][r], pre_kn[k][r], pre_kw[k], pre_ka, pre_kb);
            }
            *reinterpret_cast<floatx4*>(a.xs + (size_t)ot.pix * COUT + ot.m) = xn;
            if constexpr ((EPI & EPI_GUIDE) != 0) *reinterpret_cast<floatx4*>(a.y + (size_t)ot.pix * COUT + ot.m) = xn;
        } else if constexpr ((EPI & EPI_DDIM) != 0) {
            // noise_pred = o; the reverse update of model.py:442-458 (ddim_update, one rounding per op)
            const floatx4 xv = pre_s[k];
            floatx4 xn;
            const size_t hw = (size_t)a.Hout * a.Wout;
            const size_t lbase = ((size_t)ot.b * COUT + ot.m) * hw + (size_t)ot.oy * a.Wout + ot.ox;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float x0;
                xn[r] = ddim_update(xv[r], o[r], a.coef, a.eta, x0);
                if (a.x0_log) a.x0_log[lbase + r * hw] = x0;
                if (a.eps_log) a.eps_log[lbase + r * hw] = o[r];
            }
            if constexpr ((EPI & EPI_KEEP) != 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) xn[r] = keep_blend(xn[r], pre_kz[k][r], pre_kn[k][r], pre_kw[k], pre_ka, pre_kb);
            }
            *reinterpret_cast<floatx4*>(a.xs + (size_t)ot.pix * COUT + ot.m) = xn;
            if constexpr ((EPI & EPI_GUIDE) != 0) *reinterpret_cast<floatx4*>(a.y + (size_t)ot.pix * COUT + ot.m) = xn;
        } else {
            *reinterpret_cast<floatx4*>(a.y + (size_t)ot.pix * COUT + ot.m) = o;
        }
    });
    UCONV_STAMP(4);
}

// The plain step kernel: one layer per launch.
template <int MODE, int CIN, int COUT, int TM, int TN, int WN, int WK, int NCH, int S, int EPI, int DT, int KS = 1>
__global__ __launch_bounds__(64 * WN * WK) __attribute__((amdgpu_waves_per_eu((WN * WK + 3) / 4, (WN * WK + 3) / 4)))
void uconv_kernel(const float* w, const float* x, int32_t xbytes, uint32_t dec, int32_t tiles, int32_t Nq, int32_t Hin,
                  int32_t Win, uint32_t mul_hw, uint32_t mul_w, uint32_t shr, UArgs a) {
    const UHead h{w, x, xbytes, dec, tiles, Nq, Hin, Win, mul_hw, mul_w, shr};   // (see UHead: the preloaded parameters)
    if constexpr (KS == kTapClass) {
        // blocks [0, tiles): tap class 1, [tiles, 2 tiles): class 2 — the two blocks of a tile are a whole number of
        // XCD rounds apart (tile counts that are multiples of 8), so they read the tile's activations from one L2.
        // NCH / S are class 2's chunk counts (5 taps per channel chunk); class 1 runs 4 per channel chunk.
        if ((int)blockIdx.x < h.tiles)
            uconv_body<MODE, CIN, COUT, TM, TN, WN, WK, NCH / 5 * 4, S / 5 * 4, EPI, DT, 1, 1>(h, a, blockIdx.x);
        else
            uconv_body<MODE, CIN, COUT, TM, TN, WN, WK, NCH, S, EPI, DT, 1, 2>(h, a, (int)blockIdx.x - h.tiles);
    } else {
        uconv_body<MODE, CIN, COUT, TM, TN, WN, WK, NCH, S, EPI, DT, KS>(h, a, blockIdx.x);
    }
}

// XCD-grid block order (order 2 in set_grid); LDM_UCONV_XCD=0 turns it off for A/B timing (uconv.hip reads it)
bool xcd_grid();

// The split-K workspace as uconv.hip's tables size it for the form being launched (ks_tiles, step_ws_floats): an
// instance with KS > 1 takes its counters and slabs from it after checking its own tile count against the table's.
struct KsWs {
    float* ws = nullptr;
    int64_t tiles = 0, slab_floats = 0, cnt_floats = 0, ws_floats = 0;
};

// The launch arguments that depend on the tile shape, from the constants the kernel is instantiated with (make_args,
// uconv.hip, fills the rest): the tile counts, the block order and, for KS > 1, the workspace pointers.
template <int CIN, int COUT, int TM, int TN, int WN, int KS>
static int set_grid(UArgs& a, const KsWs& k) {
    constexpr int bm = 16 * TM, bn = 16 * TN * WN;
    a.nMt = COUT / bm;
    a.nNt = (a.Nq + bn - 1) / bn;
    // weight-heavy layers keep one M tile's blocks together (N tile fastest would spread a weight slab
    // over every XCD's L2); activation-heavy ones walk M fastest
    const int64_t wbytes = (int64_t)9 * CIN * COUT * 4, xbytes = (int64_t)a.B * a.Hin * a.Win * CIN * 4;
    a.order = wbytes > xbytes ? 0 : 1;
    // XCD grid (order 2, LDM_UCONV_XCD=0 keeps orders 0 / 1): the split of the 8 XCDs over (M, N) tiles with
    // the fewest bytes fetched into the eight L2s, xpn x weights + xpm x input (each XCD its weight and input
    // slices; contiguous N slices share their halo rows); only where both tile counts divide
    if (xcd_grid() && ((int64_t)a.nMt * a.nNt) % 8 == 0) {
        int64_t best = -1;
        for (int pm = 1; pm <= 8; pm *= 2) {
            const int pn = 8 / pm;
            if (a.nMt % pm || a.nNt % pn) continue;
            const int ml = a.nMt / pm;   // (the kernel decodes with shifts: whole powers of two, nNt / xpn in 24 bits)
            if ((ml & (ml - 1)) != 0 || ml > (1 << 15) || a.nNt / pn >= (1 << 24)) continue;
            const int64_t est = pn * wbytes + pm * xbytes;
            if (best < 0 || est < best) best = est, a.xpm = pm, a.xpn = pn;
        }
        if (best >= 0) a.order = 2;
    }
    a.fd_mt = FastDiv::make(a.nMt);
    a.fd_nt = FastDiv::make(a.nNt);
    a.fd_tiles = FastDiv::make(a.nMt * a.nNt);
    if constexpr (KS > 1) {   // (the tap-class form, KS = kTapClass, leaves no partial tiles: slab and cnt stay null)
        LDM_REQUIRE(k.ws && k.tiles == (int64_t)a.nMt * a.nNt && k.ws_floats >= k.cnt_floats + k.slab_floats &&
                        (k.cnt_floats + k.slab_floats) * 4 < 0x7fffffffLL,
                    "step conv: split-K workspace geometry");
        a.cnt = reinterpret_cast<int32_t*>(k.ws);
        a.slab = k.ws + k.cnt_floats;
    }
    return 0;
}

// The head record of a launch from its finished arguments (make_args and set_grid have run).
static inline UHead make_head(const UArgs& a, int cin) {
    auto log2u = [](int v) {
        uint32_t l = 0;
        while ((1 << l) < v) ++l;
        return l;
    };
    UHead h{};
    h.w = a.w;
    h.x = a.x;
    h.xbytes = a.B * a.Hin * a.Win * cin * 4;
    h.dec = (uint32_t)a.order;
    if (a.order == 2) h.dec |= log2u(a.xpn) << 2 | log2u(a.nMt / a.xpm) << 4 | (uint32_t)(a.nNt / a.xpn) << 8;
    h.tiles = a.nMt * a.nNt;
    h.Nq = a.Nq;
    h.Hin = a.Hin;
    h.Win = a.Win;
    h.mul_hw = a.fd_hw.mul;
    h.mul_w = a.fd_w.mul;
    h.shr = a.fd_hw.shr | (a.fd_hw.one & 1u) << 5 | a.fd_w.shr << 8 | (a.fd_w.one & 1u) << 13;
    return h;
}

template <int MODE, int CIN, int COUT, int TM, int TN, int WN, int WK, int NCH, int S, int EPI, int DT, int KS>
static int launch_dt(const UArgs& a, hipStream_t st) {
    // (tap classes: sized for class 2, the larger of the two: three parities, S / 5 channel chunks per wave)
    constexpr int NPH = KS == kTapClass ? tc_nph(MODE, 2) : tc_nph(MODE, 0);
    constexpr int NCC = KS == kTapClass ? S / 5 : S / 9;
    const int blocks = a.nMt * a.nNt * (KS == kTapClass ? 2 : KS);
    size_t lds = std::max<size_t>(WK > 1 ? (size_t)WK * WN * NPH * TM * TN * 64 * 16 : 0, KS > 1 ? 16 : 0);
    if constexpr ((EPI & EPI_PLANE) != 0)   // + each wave's activation window (see EPI_PLANE; 4 KB per sample at stride 2)
        lds = (WK > 1 ? (size_t)WK * WN * NPH * TM * TN * 64 * 16 : 0) + (size_t)WN * WK * NCC * TN * (MODE == 1 ? 4096 : 1024);
    if constexpr ((EPI & EPI_WINDOW) != 0) {   // + each wave's row window (see EPI_WINDOW)
        constexpr int WR = MODE == 2 ? 2 : 3;
        constexpr int WC = MODE == 0 ? 16 * TN + 2 : (MODE == 1 ? 32 * TN + 1 : 16 * TN + 1);
        lds = (WK > 1 ? (size_t)WK * WN * NPH * TM * TN * 64 * 16 : 0) + (size_t)WN * WK * NCC * WR * WC * 64;
    }
    auto kfn = uconv_kernel<MODE, CIN, COUT, TM, TN, WN, WK, NCH, S, EPI, DT, KS>;
    if (lds > 64 * 1024) {   // dynamic LDS past 64 KiB needs the per-function opt-in, once
        static bool opted = false;
        if (!opted) {
            LDM_HIP_TRY(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            opted = true;
        }
    }
    const UHead h = make_head(a, CIN);
    hipLaunchKernelGGL(kfn, dim3((unsigned)blocks), dim3(64 * WN * WK), lds, st, h.w, h.x, h.xbytes, h.dec, h.tiles, h.Nq, h.Hin,
                       h.Win, h.mul_hw, h.mul_w, h.shr, a);
    LDM_CHECK_LAUNCH("uconv_kernel");
    return 0;
}

// operand precision (StepConv::dtype) -> instance, on the grid of that instance (set_grid)
template <int MODE, int CIN, int COUT, int TM, int TN, int WN, int WK, int NCH, int S, int EPI, int KS = 1>
static int launch(UArgs a, int dtype, hipStream_t st, const KsWs& k = {}) {
    if (int rc = set_grid<CIN, COUT, TM, TN, WN, KS>(a, k)) return rc;
    switch (dtype) {
        case LDM_DT_F32: return launch_dt<MODE, CIN, COUT, TM, TN, WN, WK, NCH, S, EPI, 0, KS>(a, st);
        case LDM_DT_F16: return launch_dt<MODE, CIN, COUT, TM, TN, WN, WK, NCH, S, EPI, 1, KS>(a, st);
        case LDM_DT_BF16: return launch_dt<MODE, CIN, COUT, TM, TN, WN, WK, NCH, S, EPI, 2, KS>(a, st);
        default: return fail(2, "step conv: unknown operand precision");
    }
}

// dec1's five geometries, stated here only: {tm, tn, wn, wk, nch, s, EPI_WINDOW or 0} of launch<>.  uconv.hip's
// dec1_geo picks the index.
struct Dec1Geo {
    int tm, tn, wn, wk, nch, s, flag;
};
constexpr Dec1Geo kDec1Geo[5] = {
    {1, 2, 2, 4, 9, 9, EPI_WINDOW},     // 0: variant 3, windowed: 16 x 64 tiles (2 wave columns), K over 4 waves
    {1, 2, 2, 2, 18, 18, EPI_WINDOW},   // 1: the thin form (16 of the 32 rows x 64 positions, K over 2 waves), windowed
    {1, 2, 2, 2, 18, 18, 0},            // 2: the thin form
    {2, 2, 1, 4, 9, 9, EPI_WINDOW},     // 3: the 32-row form, windowed
    {2, 2, 1, 4, 9, 9, 0},              // 4: the 32-row form
};
// the instance with epilogue bits EPI on geometry GEO
template <int EPI, int GEO>
static int dec1_launch(const UArgs& a, int dtype, hipStream_t st) {
    constexpr Dec1Geo g = kDec1Geo[GEO];
    return launch<0, 64, 32, g.tm, g.tn, g.wn, g.wk, g.nch, g.s, EPI | g.flag>(a, dtype, st);
}
// f(integral_constant<int, geo>): a dispatcher's choice of epilogue bits, written once over GEO, on the run-time geometry
template <class F>
static int dec1_visit(int geo, F&& f) {
    switch (geo) {
        case 0: return f(std::integral_constant<int, 0>{});
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        default: return fail(2, "step conv: unknown dec1 geometry");
    }
}

// dec1's two launches in the guided loop live in a translation unit of their own (uconv_guide.hip), so that the code
// object of the unguided step kernels holds exactly the instances it held without guidance: the base
// half as a plain conv, or the target half with the guided DDIM / multistep update
int step_dec1_guided(int geo, const UArgs& a, const StepConv& s, hipStream_t st);
// dec1 with the regional keep, guided or not, likewise (uconv_keep.hip); the guided loop's plain base half stays
// step_dec1_guided's
int step_dec1_keep(int geo, const UArgs& a, const StepConv& s, hipStream_t st);

}  // namespace uc
}  // namespace ldm
