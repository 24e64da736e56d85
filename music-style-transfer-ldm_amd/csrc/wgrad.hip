// Conv / transposed-conv weight gradient of the train step (LDMTrainer.train_step, train.py:163-208:
// scaler.scale(loss).backward() through every trained conv) as a tap-shared implicit GEMM for gfx950.
//
//   dW[m][c][t] = sum_{b,q} Dense[b][m][q] * Gath[b][c][q*s + d_t],   d_t = (kh - pad, kw - pad)
//   conv  (w [Cout][Cin][k][k]):  Dense = dY (m = co, q over Hout x Wout), Gath = X,  s = stride
//   convT (w [Cin][Cout][k][k]):  Dense = X  (m = ci, q over Hin  x Win ), Gath = dY, s = stride
//
// One block owns a BM (m) x BC (c) tile for ALL k*k taps and walks a slice of K = (b, q) in chunks of 64
// output positions (one 64-wide row segment, or 64/Wq whole rows).  Per chunk it DMAs into LDS (16 B per
// lane, buffer_load ... lds) the Dense rows [BM][64] and the Gath window the chunk's taps touch,
// [BC][WR][WCa] (borders and channels past C arrive as zeros: the window origin is aligned down to 4
// floats, so a 16-B piece is either inside the image row or wholly outside it).  Every Dense fragment is
// then read once per 16 positions and reused by all k*k taps, every window value by every tap that
// covers it: the previous kernel (backward.hip) gathered 4 scalars per lane per tap from global memory.
// Chunks are double-buffered: the DMAs of chunk i+1 are issued before chunk i is multiplied.
// K is split over blocks (grid.z) into fixed ranges; wgrad_reduce_kernel sums the partials in split
// order, so the result is bitwise reproducible.
// MFMA v_mfma_f32_16x16x4_f32: lane l = (col l&15, group g = l>>4); for the 16 positions of step u the
// lane supplies positions 16u + 4g + j at MFMA j (A as one float4 from LDS, B as 4 window values).
//
// Kernels of this file:
//   wgrad_kernel, wgrad_c1_kernel   the tap-shared form above (fp32 MFMA, or 16-bit operands four positions a step)
//   wgrad_ring_kernel<.., EB, NBUF> the double-rate 16-bit-operand form on an NBUF-deep LDS-DMA ring of chunks; both
//                                   maps stored in EB bytes an element (4: fp32, 2: fp16 / bf16).  The train step.
//   wgrad_staged_kernel             the same sums with the tiles staged through registers and plain __syncthreads:
//                                   either map fp32 or 16-bit (mixed storage), LDM_WGRAD_RING=2, and the form the
//                                   ring is compared with bit for bit.
#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "common.h"

#pragma clang fp contract(off)

namespace ldm {
namespace wg {

struct Args {
    const float* dense;   // [B][M][Hq*Wq]
    const float* gath;    // [B][C][Hg][Wg]
    float* partial;       // [S][M][C*T]
    int32_t B, M, C, Hq, Wq, Hg, Wg, pad;
    int32_t cols, rows;   // chunk = rows x cols output positions (cols = min(Wq, 64), rows = 64 / cols)
    int32_t cps;          // chunks per sample
    int32_t nchunk, per_split;
    int32_t wr, wca, e;   // window rows, row pitch (floats, multiple of 4), column shift of the aligned origin
    int32_t pitch_c;      // floats per channel in the window (wr * wca)
    int32_t lowp;         // LDM_DT_*: operands rounded to fp16 / bf16, fp32 accumulation
    int32_t dense16;      // wgrad_c1_kernel XS != 0: Dense stored in 16 bits (register-staged, see wgrad_staged_kernel)
};

template <int B_, int E_, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (B_ < E_) {
        f(std::integral_constant<int, B_>{});
        static_for<B_ + 1, E_>(f);
    }
}

typedef __attribute__((address_space(3))) void* lds_ptr_t;
constexpr int kOOB = 0x7ffffff0;
constexpr int kKQ = 64;   // output positions per chunk
constexpr int kLdsMax = 160 * 1024;   // LDS of a CU: the most a block's buffers may take

// chunk ch -> (sample, first output row, first output column): a chunk is a.rows whole rows (cols == Wq), or one
// seg-wide segment of a row
template <class A>
__device__ __forceinline__ void chunk_origin(const A& a, int seg, int ch, int& b, int& qy0, int& qx0) {
    b = ch / a.cps;
    const int r = ch - b * a.cps;
    if (a.cols == a.Wq) {
        qy0 = r * a.rows, qx0 = 0;
    } else {
        const int segs = a.Wq / seg;
        qy0 = r / segs, qx0 = (r - qy0 * segs) * seg;
    }
}

template <class V, int N0, int N1>
__device__ __forceinline__ void clear_acc(V (&acc)[N0][N1]) {
#pragma unroll
    for (int i = 0; i < N0; ++i)
#pragma unroll
        for (int j = 0; j < N1; ++j) acc[i][j] = V{};
}

// Opts kfn into the whole LDS as dynamic shared memory on its first call, then launches it.
template <auto kfn, class A>
int launch_lds(const char* name, dim3 grid, int threads, int lds_bytes, hipStream_t st, const A& a) {
    static bool opted = false;
    if (!opted) {
        LDM_HIP_TRY(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
        opted = true;
    }
    hipLaunchKernelGGL(kfn, grid, dim3(threads), lds_bytes, st, a);
    LDM_CHECK_LAUNCH(name);
    return 0;
}

// M = rows of dW (Dense channels), C = gathered channels; the Dense plane Hq x Wq, the gathered plane Hg x Wg
template <class A>
void conv_dims(const ldm_conv_desc& d, A& a) {
    a.B = d.B;
    if (!d.transposed) {
        a.M = d.Cout, a.C = d.Cin, a.Hq = d.Hout, a.Wq = d.Wout, a.Hg = d.Hin, a.Wg = d.Win;
    } else {
        a.M = d.Cin, a.C = d.Cout, a.Hq = d.Hin, a.Wq = d.Win, a.Hg = d.Hout, a.Wg = d.Wout;
    }
}

template <int S, int KK, int BM, int BC>
struct Cfg {
    static constexpr int T = KK * KK;
    static constexpr int WCF = BC / 16, WMF = 4 / WCF, FM = BM / 16 / WMF;   // 4 waves: WMF x WCF, FM m-frags each
    static_assert(WMF * WCF == 4 && FM >= 1 && FM * 16 * WMF == BM, "wave layout");
    static constexpr int A_FLOATS = BM * kKQ;
};

// floats of one LDS buffer: A rows + the window rounded up to whole wave-instructions (64 pieces)
__host__ __device__ inline int buf_floats(int a_floats, int bc, int pitch_c) {
    return a_floats + (bc * pitch_c + 255) / 256 * 256;
}

template <int S, int KK, int BM, int BC, int DT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void wgrad_kernel(Args a) {
    using g = Cfg<S, KK, BM, BC>;
    constexpr int T = g::T, WCF = g::WCF, FM = g::FM, AF = g::A_FLOATS;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wc = wave % WCF, wm = wave / WCF;
    const int col = lane & 15, lg = lane >> 4;
    const int m0 = blockIdx.y * BM, c0 = blockIdx.x * BC;
    const int HQ = a.Hq * a.Wq;
    const int bufF = buf_floats(AF, BC, a.pitch_c);
    const int ch_begin = blockIdx.z * a.per_split;
    const int ch_end = min(a.nchunk, ch_begin + a.per_split);

    const __amdgpu_buffer_rsrc_t dr = __builtin_amdgcn_make_buffer_rsrc(
        uni_ptr(a.dense), (short)0, uni(a.B * a.M * HQ * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t gr = __builtin_amdgcn_make_buffer_rsrc(
        uni_ptr(a.gath), (short)0, uni(a.B * a.C * a.Hg * a.Wg * 4), 0x00020000);

    // DMA of chunk ch into buffer buf: A = BM rows x 64 positions (XOR-swizzled 16-B pieces), then the
    // window [BC][wr][wca]; the work is dealt round-robin over all 256 lanes' 16-B pieces.
    auto issue = [&](int ch, int buf) {
        int b, qy0, qx0;
        chunk_origin(a, kKQ, ch, b, qy0, qx0);
        char* base = reinterpret_cast<char*>(smem + buf * bufF);
        // A: BM*16 pieces = BM/4 wave-instructions
        for (int gi = wave; gi < BM / 4; gi += 4) {
            const int row = gi * 4 + (lane >> 4);
            const int p = lane & 15;                       // destination piece
            const int sp = p ^ (row & 15);                  // source piece
            const int m = m0 + row;
            const int ql = sp * 4;                          // chunk-local position of the piece
            const int qy = qy0 + ql / a.cols, qx = qx0 + ql % a.cols;
            const bool ok = m < a.M && qy < a.Hq;
            const int voff = ok ? (((b * a.M + m) * HQ + qy * a.Wq + qx) * 4) : kOOB;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(dr, (lds_ptr_t)(base + gi * 1024), 16, voff, 0, 0, 0);
        }
        // window: BC * wr * wca / 4 pieces
        const int wq4 = a.wca >> 2;
        const int npiece = BC * a.wr * wq4;
        const int row0 = qy0 * S - a.pad, colA = qx0 * S - a.pad - a.e;
        for (int gi = wave; gi * 64 < npiece; gi += 4) {
            const int pc = gi * 64 + lane;
            const int cl = pc / (a.wr * wq4);
            const int rem = pc - cl * (a.wr * wq4);
            const int wrow = rem / wq4, wp = rem - wrow * wq4;
            const int c = c0 + cl, iy = row0 + wrow, ix = colA + wp * 4;
            const bool ok = pc < npiece && c < a.C && (unsigned)iy < (unsigned)a.Hg && (unsigned)ix < (unsigned)a.Wg;
            const int voff = ok ? ((((b * a.C + c) * a.Hg + iy) * a.Wg + ix) * 4) : kOOB;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(gr, (lds_ptr_t)(base + AF * 4 + gi * 1024), 16, voff, 0, 0, 0);
        }
    };

    floatx4 acc[T][FM];
    clear_acc(acc);

    // per-lane LDS offsets inside a buffer: A row pieces, window column of position 16u + 4g (+ j*S)
    int aoff[FM][4];
#pragma unroll
    for (int f = 0; f < FM; ++f)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = (wm * FM + f) * 16 + col;
            aoff[f][u] = row * kKQ + (((4 * u + lg) ^ (row & 15)) << 2);
        }
    int boff[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        // positions past the chunk's rows (a small image zero-padded to 64) multiply zeros of A: point them
        // at position 0 so that they read finite window values (0 * NaN from stale LDS would be NaN)
        const int ql = (16 * u + 4 * lg < a.rows * a.cols) ? 16 * u + 4 * lg : 0;
        const int rl = ql / a.cols, xl = ql - rl * a.cols;
        boff[u] = AF + (wc * 16 + col) * a.pitch_c + rl * S * a.wca + a.e + xl * S;
    }

    if (ch_begin < ch_end) issue(ch_begin, 0);
    for (int ch = ch_begin; ch < ch_end; ++ch) {
        const int buf = (ch - ch_begin) & 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();   // chunk ch landed everywhere; every wave is done with the other buffer
        if (ch + 1 < ch_end) issue(ch + 1, buf ^ 1);
        const float* sb = smem + buf * bufF;
        {   // DT = operand precision (compile time: a runtime branch between MFMA forms miscompiled in conv.hip)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                floatx4 fa[FM];
#pragma unroll
                for (int f = 0; f < FM; ++f) fa[f] = *reinterpret_cast<const floatx4*>(sb + aoff[f][u]);
                static_for<0, T>([&](auto tc) {
                    constexpr int t = decltype(tc)::value;
                    constexpr int ky = t / KK, kx = t % KK;
                    const float* bp = sb + boff[u] + ky * a.wca + kx;
                    floatx4 bv;
#pragma unroll
                    for (int j = 0; j < 4; ++j) bv[j] = bp[j * S];
                    if constexpr (DT == 0) {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
#pragma unroll
                            for (int f = 0; f < FM; ++f)
                                acc[t][f] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[f][j], bv[j], acc[t][f], 0, 0, 0);
                    } else {
#pragma unroll
                        for (int f = 0; f < FM; ++f) acc[t][f] = mma16_lowp<DT>(fa[f], bv, acc[t][f]);
                    }
                });
            }
        }
    }

    // partial tile: rows m = m0 + 16*(wm*FM+f) + 4g + r, column c = c0 + 16*wc + col, T taps contiguous
    const int N = a.C * T;
    const int c = c0 + wc * 16 + col;
    if (c < a.C) {
        float* out = a.partial + (size_t)blockIdx.z * a.M * N;
#pragma unroll
        for (int f = 0; f < FM; ++f)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + (wm * FM + f) * 16 + 4 * lg + r;
                if (m < a.M) {
                    float* o = out + (size_t)m * N + (size_t)c * T;
#pragma unroll
                    for (int t = 0; t < T; ++t) o[t] = acc[t][f][r];
                }
            }
    }
}

// One gathered channel (C = 1: the Cin = 1 first layers of the VAE / style encoders, and the decoder's
// 64 -> 1 output convT): the N dimension of the GEMM is the k*k taps instead of 16 channels (the general
// kernel spent 15/16 of its window DMAs and MFMAs on padding channels there).  Block = 4 waves x 16 rows
// (m) x 16 columns (taps; k = 3 leaves 7 idle); the lane of column t reads its tap's window value, so the
// whole 16 x 16 x (64 positions) product of a chunk is 4 (16 in f32) MFMAs per wave.
template <int S, int KK, int DT, int XS = 0>
__global__ __launch_bounds__(256) void wgrad_c1_kernel(Args a) {
    constexpr int T = KK * KK, BM = 64, AF = BM * kKQ;
    static_assert(T <= 16, "taps per column tile");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 15, lg = lane >> 4;
    const int m0 = blockIdx.y * BM;
    const int HQ = a.Hq * a.Wq;
    const int bufF = buf_floats(AF, 1, a.pitch_c);
    const int ch_begin = blockIdx.z * a.per_split;
    const int ch_end = min(a.nchunk, ch_begin + a.per_split);
    const bool d16 = XS != 0 && a.dense16;
    const __amdgpu_buffer_rsrc_t dr = __builtin_amdgcn_make_buffer_rsrc(
        uni_ptr(a.dense), (short)0, uni(a.B * a.M * HQ * (d16 ? 2 : 4)), 0x00020000);
    const __amdgpu_buffer_rsrc_t gr = __builtin_amdgcn_make_buffer_rsrc(
        uni_ptr(a.gath), (short)0, uni(a.B * a.Hg * a.Wg * 4), 0x00020000);

    // XS != 0: the Dense rows register-staged (16-bit quads widened when parked at the DMA's addresses); the
    // window (the fp32 input of a Cin = 1 layer) keeps its DMA
    uint4 rd[XS ? BM / 16 : 1];
    auto fetch_dense = [&](int ch) {
        int b, qy0, qx0;
        chunk_origin(a, kKQ, ch, b, qy0, qx0);
#pragma unroll
        for (int i = 0; i < BM / 16; ++i) {
            const int gi = wave + 4 * i;
            const int row = gi * 4 + (lane >> 4);
            const int p = lane & 15;
            const int sp = p ^ (row & 15);
            const int m = m0 + row;
            const int ql = sp * 4;
            const int qy = qy0 + ql / a.cols, qx = qx0 + ql % a.cols;
            const bool ok = m < a.M && qy < a.Hq;
            const int el = ((b * a.M + m) * HQ + qy * a.Wq + qx);
            if (d16) {
                const uint2 t = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(dr, ok ? el * 2 : kOOB, 0, 0));
                rd[i] = uint4{t.x, t.y, 0u, 0u};
            } else {
                rd[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(dr, ok ? el * 4 : kOOB, 0, 0));
            }
        }
    };
    auto park_dense = [&](int buf) {
        char* base = reinterpret_cast<char*>(smem + buf * bufF);
#pragma unroll
        for (int i = 0; i < BM / 16; ++i) {
            const int gi = wave + 4 * i;
            floatx4 v;
            if (d16)
                v = floatx4{from16<XS>((unsigned short)(rd[i].x & 0xffff)), from16<XS>((unsigned short)(rd[i].x >> 16)),
                            from16<XS>((unsigned short)(rd[i].y & 0xffff)), from16<XS>((unsigned short)(rd[i].y >> 16))};
            else
                v = __builtin_bit_cast(floatx4, rd[i]);
            *reinterpret_cast<floatx4*>(base + gi * 1024 + lane * 16) = v;
        }
    };

    auto issue = [&](int ch, int buf) {
        int b, qy0, qx0;
        chunk_origin(a, kKQ, ch, b, qy0, qx0);
        char* base = reinterpret_cast<char*>(smem + buf * bufF);
        for (int gi = wave; gi < (XS ? 0 : BM / 4); gi += 4) {
            const int row = gi * 4 + (lane >> 4);
            const int p = lane & 15;
            const int sp = p ^ (row & 15);
            const int m = m0 + row;
            const int ql = sp * 4;
            const int qy = qy0 + ql / a.cols, qx = qx0 + ql % a.cols;
            const bool ok = m < a.M && qy < a.Hq;
            const int voff = ok ? (((b * a.M + m) * HQ + qy * a.Wq + qx) * 4) : kOOB;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(dr, (lds_ptr_t)(base + gi * 1024), 16, voff, 0, 0, 0);
        }
        const int wq4 = a.wca >> 2;
        const int npiece = a.wr * wq4;
        const int row0 = qy0 * S - a.pad, colA = qx0 * S - a.pad - a.e;
        for (int gi = wave; gi * 64 < npiece; gi += 4) {
            const int pc = gi * 64 + lane;
            const int wrow = pc / wq4, wp = pc - wrow * wq4;
            const int iy = row0 + wrow, ix = colA + wp * 4;
            const bool ok = pc < npiece && (unsigned)iy < (unsigned)a.Hg && (unsigned)ix < (unsigned)a.Wg;
            const int voff = ok ? (((b * a.Hg + iy) * a.Wg + ix) * 4) : kOOB;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(gr, (lds_ptr_t)(base + AF * 4 + gi * 1024), 16, voff, 0, 0, 0);
        }
    };

    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
    int aoff[4], boff[4];
    const int row = wave * 16 + col;
    const int tcol = col < T ? col : 0;   // idle columns (k = 3) re-read tap 0; their results are dropped
    const int ky = tcol / KK, kx = tcol - ky * KK;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        aoff[u] = row * kKQ + (((4 * u + lg) ^ (row & 15)) << 2);
        const int ql = (16 * u + 4 * lg < a.rows * a.cols) ? 16 * u + 4 * lg : 0;
        const int rl = ql / a.cols, xl = ql - rl * a.cols;
        boff[u] = AF + (rl * S + ky) * a.wca + a.e + xl * S + kx;
    }

    if (ch_begin < ch_end) {
        issue(ch_begin, 0);
        if constexpr (XS != 0) {
            fetch_dense(ch_begin);
            park_dense(0);
        }
    }
    for (int ch = ch_begin; ch < ch_end; ++ch) {
        const int buf = (ch - ch_begin) & 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (ch + 1 < ch_end) {
            issue(ch + 1, buf ^ 1);
            if constexpr (XS != 0) fetch_dense(ch + 1);
        }
        const float* sb = smem + buf * bufF;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const floatx4 fa = *reinterpret_cast<const floatx4*>(sb + aoff[u]);
            floatx4 bv;
#pragma unroll
            for (int j = 0; j < 4; ++j) bv[j] = sb[boff[u] + j * S];
            if constexpr (DT == 0) {
#pragma unroll
                for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[j], bv[j], acc, 0, 0, 0);
            } else {
                acc = mma16_lowp<DT>(fa, bv, acc);
            }
        }
        if constexpr (XS != 0) {
            if (ch + 1 < ch_end) park_dense(buf ^ 1);
        }
    }
    // D: row m = m0 + 16*wave + 4*lg + r, column = tap col
    if (col < T) {
        float* out = a.partial + (size_t)blockIdx.z * a.M * T;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + wave * 16 + 4 * lg + r;
            if (m < a.M) out[(size_t)m * T + col] = acc[r];
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// The same weight gradient with 16-bit operands (the train step's torch.autocast region) on the gfx950
// double-rate v_mfma_f32_32x32x16_{f16,bf16}: K = 16 positions per MFMA instead of 4 per f32 MFMA.
//
// The fp32 form above reads its gathered operand one scalar per position per tap, so at 16-bit rates
// it would be bound by LDS reads and their conversions.  Here a block owns BM rows (m) x 32 gathered
// channels (c) x all k*k taps; its NW = WM * KK waves split the rows (wm) and the tap rows (ky): a wave
// covers BM/WM rows and the KK taps (ky, 0..KK-1) of 32 channels.  K is walked in chunks of QC = 32 output
// positions (one 32-wide row segment, or two 16-wide rows; two MFMA k-steps of 16 positions each) or QC = 16
// (one k-step: the 2 x 8 planes of the UNet bottom).  Requires pad = 1 (every k3 / k4 layer of the model).
//
// A chunk's tiles lie in LDS as their maps store them, in elements of EB bytes (4: fp32, 2: fp16 / bf16), PE =
// 16 / EB elements to the 16-byte piece:
//   Dense  [BM][QC], the pieces of a row XOR-swizzled per row pair (lp_swz);
//   window [32][pitch_c]: per channel wr rows of wca elements from the PE-aligned origin qx0*S - 1 - E, E = PE - 1
//          (Wg % PE == 0, so a piece is wholly inside or outside the image row; borders and channels past C
//          arrive as zeros); the channel pitch is PE mod 16 PE elements (16 B mod 256 B: 16 lanes' 16-byte reads
//          are conflict-free).
// Per k-step a lane of column c needs positions q0 .. q0+7 (q0 = 16 ks + 8 h) of every kx tap, i.e. window
// elements E + kx + S j of one window row; their union is one aligned run of NB pieces, read as NB ds_read_b128,
// and lp_cut takes each tap's fragment from it: from fp32 maps 8 of those registers, rounded to the operand type
// at the MFMA; from 16-bit maps 8 halves picked without any conversion (stride 2: one v_perm per dword, stride 1:
// aligned, or a funnel shift).  The Dense fragment is the 8 positions' EB / 2 pieces.  Both element widths walk
// the same blocks, chunks, k-steps and MFMAs, so on the same values their sums are bitwise equal.
// MFMA maps (cdna_hip_programming.md §3): lane l (r = l & 31, h = l >> 5) holds A[row r][k = 8h + j] and
// B[k = 8h + j][col r]; D col = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4h.
// ------------------------------------------------------------------------------------------------------
constexpr int kLC = 32;    // gathered channels per block
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 halfx8 __attribute__((ext_vector_type(8)));
typedef float floatx8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct LpArgs {
    const float* dense;   // [B][M][Hq*Wq]
    const float* gath;    // [B][C][Hg][Wg]
    float* partial;       // [splits][M][C*T]
    int32_t B, M, C, Hq, Wq, Hg, Wg;
    int32_t cols, rows, cps, nchunk, per_split;
    int32_t wr, wca, pitch_c;   // window rows, row pitch, channel pitch (elements of the LDS tile)
    int32_t dense16, gath16;    // wgrad_staged_kernel: dense / gath stored in 16 bits
};

// ---- the tile geometry of an element width eb (bytes), host and device
__host__ __device__ constexpr int lp_wca(int eb, int S, int KK, int cols) {
    const int pe = 16 / eb;
    return (pe - 1 + (cols - 1) * S + KK + pe - 1) / pe * pe;
}
__host__ __device__ constexpr int lp_pitch(int eb, int S, int KK, int rows, int cols) {
    const int pe = 16 / eb;
    int pc = ((rows - 1) * S + KK) * lp_wca(eb, S, KK, cols);
    while (pc % (16 * pe) != pe) pc += pe;
    return pc;
}
// the larger of the two chunk geometries a QC allows (one row of QC positions, two rows of QC / 2)
__host__ __device__ constexpr int lp_pitch_max(int eb, int S, int KK, int QC) {
    const int p1 = lp_pitch(eb, S, KK, 1, QC), p2 = lp_pitch(eb, S, KK, 2, QC / 2);
    return p1 > p2 ? p1 : p2;
}
// window pieces per lane: the largest window of (S, KK, QC) dealt over the NW waves' 64 lanes
__host__ __device__ constexpr int lp_slots(int eb, int S, int KK, int QC, int NW) {
    return (kLC * (lp_pitch_max(eb, S, KK, QC) / (16 / eb)) + 64 * NW - 1) / (64 * NW);
}
__host__ __device__ constexpr int lp_nb(int eb, int S, int KK) {   // b128 reads per k-step
    const int pe = 16 / eb;
    return (pe - 1 + 7 * S + KK + pe - 1) / pe;
}
// one chunk buffer: the Dense rows + the window rounded up to whole wave-instructions (1 KB)
__host__ __device__ constexpr int lp_buf_bytes(int eb, int bm, int qc, int pitch_c) {
    return bm * qc * eb + (kLC * pitch_c * eb + 1023) / 1024 * 1024;
}
// dynamic LDS of a launch: nbuf = 2 the staged form's double buffer; 3 / 4 the ring, + its trash KB (+ at 16
// bits a tail past the last run)
__host__ __device__ constexpr int lp_lds_bytes(int eb, int nbuf, int bm, int qc, int pitch_c) {
    return nbuf * lp_buf_bytes(eb, bm, qc, pitch_c) + (nbuf == 2 ? 0 : 1024 + (eb == 2 ? 64 : 0));
}
// XOR swizzle of a Dense row's 16-B pieces (PPR per row): 16 consecutive rows' fragment reads land on
// distinct bank groups
template <int PPR>
__host__ __device__ constexpr int lp_swz(int row) { return (row >> 1) & (PPR - 1); }

template <int DT>
__device__ __forceinline__ floatx16 mma32x16(const floatx8& a, const floatx8& b, const floatx16& c) {
    if constexpr (DT == 1)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_convertvector(a, halfx8), __builtin_convertvector(b, halfx8),
                                                      c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_convertvector(a, bf16x8),
                                                       __builtin_convertvector(b, bf16x8), c, 0, 0, 0);
}
template <int DT>
__device__ __forceinline__ floatx16 mma32x16(const u16x8& a, const u16x8& b, const floatx16& c) {
    if constexpr (DT == 1)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(halfx8, a), __builtin_bit_cast(halfx8, b), c, 0,
                                                      0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c,
                                                       0, 0, 0);
}

// 8 consecutive 16-bit elements starting at element `e` (compile-time) of the dword array w, stride S
template <int S, int E, int N>
__device__ __forceinline__ u16x8 lp16_frag(const unsigned (&w)[N]) {
    static_assert((E >> 1) + (S == 2 ? 8 : 5) <= N, "fragment past the loaded run");
    unsigned d[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if constexpr (S == 2) {
            // elements E + 4i and E + 4i + 2: the same half of dwords (E + 4i) / 2 and (E + 4i) / 2 + 1
            constexpr int h = E & 1;
            const unsigned lo = w[(E >> 1) + 2 * i], hi = w[(E >> 1) + 2 * i + 1];
            d[i] = h ? ((lo >> 16) | (hi & 0xffff0000u)) : ((lo & 0xffffu) | (hi << 16));
        } else {
            if constexpr ((E & 1) == 0) {
                d[i] = w[(E >> 1) + i];
            } else {
                const unsigned lo = w[(E >> 1) + i], hi = w[(E >> 1) + i + 1];
                d[i] = (lo >> 16) | (hi << 16);
            }
        }
    }
    return __builtin_bit_cast(u16x8, (uint4){d[0], d[1], d[2], d[3]});
}

// The fragment cut.  B of tap column KX for positions q0 + j: elements E + KX + S j of the lane's loaded run w
// (dwords); A: the 8 positions' pieces.  fp32 maps give floats (rounded in mma32x16), 16-bit maps the operand itself.
template <int EB, int S, int KX, int N>
__device__ __forceinline__ auto lp_cut(const unsigned (&w)[N]) {
    if constexpr (EB == 4) {
        floatx8 fb;
#pragma unroll
        for (int j = 0; j < 8; ++j) fb[j] = __builtin_bit_cast(float, w[3 + KX + S * j]);
        return fb;
    } else {
        return lp16_frag<S, 7 + KX, N>(w);
    }
}
template <int EB>
__device__ __forceinline__ auto lp_dense_frag(const u32x4 (&ra)[EB / 2]) {
    if constexpr (EB == 4) {
        const floatx4 lo = __builtin_bit_cast(floatx4, ra[0]), hi = __builtin_bit_cast(floatx4, ra[1]);
        return floatx8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    } else {
        return __builtin_bit_cast(u16x8, ra[0]);
    }
}

// partial[z][m][c*T + ky*KK + kx]: D col = channel c, rows (reg & 3) + 8 (reg >> 2) + 4h of fragment f from row mf0
template <int KK, int MF>
__device__ __forceinline__ void lp_store_partial(const LpArgs& a, const floatx16 (&acc)[MF][KK], int mf0, int c, int ky, int h) {
    constexpr int T = KK * KK;
    if (c < a.C) {
        float* out = a.partial + (size_t)blockIdx.z * a.M * a.C * T + (size_t)c * T + ky * KK;
#pragma unroll
        for (int f = 0; f < MF; ++f)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int m = mf0 + f * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
                if (m < a.M) {
                    float* o = out + (size_t)m * a.C * T;
                    if constexpr (KK == 4) {
                        *reinterpret_cast<floatx4*>(o) = floatx4{acc[f][0][reg], acc[f][1][reg], acc[f][2][reg], acc[f][3][reg]};
                    } else {
#pragma unroll
                        for (int kx = 0; kx < KK; ++kx) o[kx] = acc[f][kx][reg];
                    }
                }
            }
    }
}

// The register-staged form: either map fp32 or 16-bit, told per tensor at run time (a DMA cannot widen 16-bit
// elements).  The tiles are fp32 in LDS (the EB = 4 geometry): the next chunk's pieces are loaded into registers
// during this chunk's MFMAs, widened and parked in LDS, double-buffered under plain __syncthreads; the compute side
// reads them with ordinary loads.  It serves the mixed-storage calls of the C ABI and LDM_WGRAD_RING=2, and is what
// the ring's sums are compared with bit for bit: the same blocks, chunks, k-steps, fragments and MFMA order, none of
// the ring's counted waits.
template <int S, int KK, int BM, int WM, int QC, int DT>
__global__ __launch_bounds__(64 * WM * KK) void wgrad_staged_kernel(LpArgs a) {
    constexpr int NW = WM * KK, MF = BM / WM / 32, NB = lp_nb(4, S, KK);
    constexpr int PPR = QC / 4, RPI = 64 / PPR, NKS = QC / 16;   // pieces per row, rows per wave-instruction, k-steps
    static_assert(MF >= 1 && MF * 32 * WM == BM, "row split");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ky = wave % KK, wm = wave / KK;
    const int r = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.y * BM, c0 = blockIdx.x * kLC;
    const int HQ = a.Hq * a.Wq;
    const int bufF = lp_buf_bytes(4, BM, QC, a.pitch_c) / 4;
    const int ch_begin = blockIdx.z * a.per_split;
    const int ch_end = min(a.nchunk, ch_begin + a.per_split);
    const bool d16 = a.dense16, g16 = a.gath16;
    const __amdgpu_buffer_rsrc_t dr = __builtin_amdgcn_make_buffer_rsrc(
        uni_ptr(a.dense), (short)0, uni(a.B * a.M * HQ * (d16 ? 2 : 4)), 0x00020000);
    const __amdgpu_buffer_rsrc_t gr = __builtin_amdgcn_make_buffer_rsrc(
        uni_ptr(a.gath), (short)0, uni(a.B * a.C * a.Hg * a.Wg * (g16 ? 2 : 4)), 0x00020000);

    // the pieces of chunk ch, loaded as 16-byte fp32 quads or 8-byte 16-bit quads and widened to floats when parked
    constexpr int ND = (BM / RPI + NW - 1) / NW, NWPC = lp_slots(4, S, KK, QC, NW);
    uint4 rd[ND], rw[NWPC];
    auto fetch = [&](int ch) {
        int b, qy0, qx0;
        chunk_origin(a, QC, ch, b, qy0, qx0);
#pragma unroll
        for (int i = 0; i < ND; ++i) {
            const int gi = wave + i * NW;
            const int row = gi * RPI + lane / PPR;
            const int sp = (lane % PPR) ^ lp_swz<PPR>(row);   // source piece landing in destination piece lane % PPR
            const int ql = sp * 4;
            const int qy = qy0 + ql / a.cols, qx = qx0 + ql % a.cols;
            const int m = m0 + row;
            const int el = ((b * a.M + m) * HQ + qy * a.Wq + qx);
            const bool ok = gi < BM / RPI && m < a.M;
            if (d16) {
                const uint2 t = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(dr, ok ? el * 2 : kOOB, 0, 0));
                rd[i] = uint4{t.x, t.y, 0u, 0u};
            } else {
                rd[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(dr, ok ? el * 4 : kOOB, 0, 0));
            }
        }
        // window [32][pitch_c]: rows of wca floats, pieces past wr * wca in a channel are padding (zeros)
        const int wq4 = a.wca >> 2, pq = a.pitch_c >> 2;
        const int npiece = kLC * pq;
        const int row0 = qy0 * S - 1, colA = qx0 * S - 4;   // pad 1, e = 3
#pragma unroll
        for (int i = 0; i < NWPC; ++i) {
            const int pc = (wave + i * NW) * 64 + lane;
            const int cl = pc / pq;
            const int rem = pc - cl * pq;
            const int wrow = rem / wq4, wp = rem - wrow * wq4;
            const int c = c0 + cl, iy = row0 + wrow, ix = colA + wp * 4;
            const bool ok = pc < npiece && c < a.C && wrow < a.wr && (unsigned)iy < (unsigned)a.Hg &&
                            (unsigned)ix < (unsigned)a.Wg;
            const int el = (((b * a.C + c) * a.Hg + iy) * a.Wg + ix);
            if (g16) {
                const uint2 t = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(gr, ok ? el * 2 : kOOB, 0, 0));
                rw[i] = uint4{t.x, t.y, 0u, 0u};
            } else {
                rw[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(gr, ok ? el * 4 : kOOB, 0, 0));
            }
        }
    };
    auto widen = [&](const uint4& v, bool h16) {
        if (!h16) return __builtin_bit_cast(floatx4, v);
        return floatx4{from16<DT>((unsigned short)(v.x & 0xffff)), from16<DT>((unsigned short)(v.x >> 16)),
                       from16<DT>((unsigned short)(v.y & 0xffff)), from16<DT>((unsigned short)(v.y >> 16))};
    };
    auto park = [&](int buf) {
        char* base = reinterpret_cast<char*>(smem + buf * bufF);
#pragma unroll
        for (int i = 0; i < ND; ++i) {
            const int gi = wave + i * NW;
            if (gi < BM / RPI) *reinterpret_cast<floatx4*>(base + gi * 1024 + lane * 16) = widen(rd[i], d16);
        }
        const int npiece = kLC * (a.pitch_c >> 2);
#pragma unroll
        for (int i = 0; i < NWPC; ++i) {
            const int gi = wave + i * NW;
            if (gi * 64 < npiece)
                *reinterpret_cast<floatx4*>(base + BM * QC * 4 + gi * 1024 + lane * 16) = widen(rw[i], g16);
        }
    };

    floatx16 acc[MF][KK];
    clear_acc(acc);

    // per-lane LDS offsets (floats) inside a buffer for k-step ks: A pieces of fragment f, window run start
    int aoff[NKS][MF][2], boff[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        const int q0 = ks * 16 + 8 * h;
        const int rl = q0 / a.cols, xl0 = q0 - rl * a.cols;
#pragma unroll
        for (int f = 0; f < MF; ++f) {
            const int row = (wm * MF + f) * 32 + r;
#pragma unroll
            for (int u = 0; u < 2; ++u) aoff[ks][f][u] = row * QC + ((((q0 >> 2) + u) ^ lp_swz<PPR>(row)) << 2);
        }
        boff[ks] = BM * QC + r * a.pitch_c + (rl * S + ky) * a.wca + xl0 * S;
    }

    auto compute = [&](const float* sb) {
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            floatx8 fa[MF];
#pragma unroll
            for (int f = 0; f < MF; ++f) {
                const u32x4 ra[2] = {*reinterpret_cast<const u32x4*>(sb + aoff[ks][f][0]),
                                     *reinterpret_cast<const u32x4*>(sb + aoff[ks][f][1])};
                fa[f] = lp_dense_frag<4>(ra);
            }
            unsigned w[4 * NB];
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const u32x4 p = *reinterpret_cast<const u32x4*>(sb + boff[ks] + 4 * i);
                w[4 * i + 0] = p[0], w[4 * i + 1] = p[1], w[4 * i + 2] = p[2], w[4 * i + 3] = p[3];
            }
            static_for<0, KK>([&](auto kxc) {
                constexpr int kx = decltype(kxc)::value;
                const floatx8 fb = lp_cut<4, S, kx>(w);
#pragma unroll
                for (int f = 0; f < MF; ++f) acc[f][kx] = mma32x16<DT>(fa[f], fb, acc[f][kx]);
            });
        }
    };
    if (ch_begin < ch_end) {
        fetch(ch_begin);
        park(0);
    }
    for (int ch = ch_begin; ch < ch_end; ++ch) {
        const int buf = (ch - ch_begin) & 1;
        __syncthreads();   // chunk ch parked by every wave; every wave is done with the other buffer
        const bool more = ch + 1 < ch_end;
        if (more) fetch(ch + 1);   // in flight during this chunk's MFMAs
        compute(smem + buf * bufF);
        if (more) park(buf ^ 1);
    }
    lp_store_partial<KK, MF>(a, acc, m0 + wm * MF * 32, c0 + r, ky, h);
}

// ------------------------------------------------------------------------------------------------------
// The ring: both maps of one element width, every tile by LDS DMA (16 B per lane, buffer_load ... lds) into an
// NBUF-deep ring of chunk buffers.  A double buffer keeps one chunk's DMAs (~25 KB per CU) in flight, which at the
// grid's one block per CU leaves the HBM pipe latency-bound; here chunks k + 1 .. k + NBUF - 1 are in flight while
// chunk k is multiplied.  Every wave issues exactly NL = ND + NG DMAs per chunk (slots past the tile's pieces load
// nothing into a trash KB), so "chunk k landed" is one vmcnt immediate; the per-slot offsets are chunk-invariant and
// computed once, and the issue cursor walks the chunk coordinates without divisions.
// Synchronisation: at iteration k the chunks k .. min(n - 1, k + NBUF - 2) are outstanding, so "chunk k landed" is
// vmcnt(ahead * NL) with ahead the chunks issued after k (a wait of one chunk less passes while chunk k is still in
// flight); then a RAW s_barrier (every wave's share of chunk k landed, every wave done reading chunk k - 1), then
// chunk k + NBUF - 1 is issued into chunk k - 1's buffer.  hipcc would drain the ring twice per chunk:
// __syncthreads()'s workgroup fence waits vmcnt(0) (an LDS DMA is a pending LDS write), and an ordinary ds_read
// after any LDS DMA waits for all of them (it may alias).  So the wait + barrier is one asm statement and the
// fragment reads are asm ds_read_b128 that end in their own lgkmcnt(0) (cdna_hip_programming.md §5, "Pipelining
// across barriers"): the emitted loop holds no vmcnt but the counted one.
// ------------------------------------------------------------------------------------------------------
// this wave's DMAs but the N youngest have landed, then the block's raw barrier (no fence: see above)
template <int N>
__device__ __forceinline__ void lp_wait_vm_barrier() {
    static_assert(N >= 0 && N <= 63, "vmcnt immediate");
    asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
}
// a ds_read_b128 the compiler's waitcnt pass does not see (the caller waits lgkmcnt(0) before the use)
__device__ __forceinline__ u32x4 lp_lds_read(const char* p) {
    u32x4 v;
    const unsigned addr = (unsigned)(uintptr_t)(lds_ptr_t)p;
    asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr));
    return v;
}

// Depth 3 fits the LDS at every chunk geometry of an instance, but for fp32 maps at k4 s2, BM 128, one 32-wide row
// (172 KB; its two-row geometry fits): lp_plan sends that one to the staged form.  Depth 4 falls back to 3.
__host__ __device__ constexpr bool lp_ring3_fits(int eb, int S, int KK, int BM, int QC) {
    return lp_lds_bytes(eb, 3, BM, QC, lp_pitch_max(eb, S, KK, QC)) <= kLdsMax;
}

template <int S, int KK, int BM, int WM, int QC, int DT, int EB, int NBUF>
__global__ __launch_bounds__(64 * WM * KK) void wgrad_ring_kernel(LpArgs a) {
    constexpr int PE = 16 / EB, LPE = EB == 4 ? 2 : 3, NA = EB / 2;   // elements per piece (and its log2), A pieces
    constexpr int NW = WM * KK, MF = BM / WM / 32, NB = lp_nb(EB, S, KK);
    constexpr int PPR = QC / PE, RPI = 64 / PPR, NKS = QC / 16;   // pieces per row, rows per DMA instr, k-steps
    constexpr int NDG = BM / RPI, ND = (NDG + NW - 1) / NW, NG = lp_slots(EB, S, KK, QC, NW), NL = ND + NG;
    static_assert(EB == 4 || EB == 2, "fp32 or 16-bit maps");
    static_assert(MF >= 1 && MF * 32 * WM == BM, "row split");
    static_assert(NBUF >= 3 && NBUF <= 4 && (NBUF - 2) * NL <= 63, "ring depth (vmcnt immediate)");
    static_assert(lp_ring3_fits(EB, S, KK, BM, QC) || (EB == 4 && S == 2 && KK == 4 && BM == 128 && QC == 32),
                  "a depth-3 ring fits the LDS");
    extern __shared__ __attribute__((aligned(16))) char smem_ring[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ky = wave % KK, wm = wave / KK;
    const int r = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.y * BM, c0 = blockIdx.x * kLC;
    const int HQ = a.Hq * a.Wq;
    const int bufB = lp_buf_bytes(EB, BM, QC, a.pitch_c);
    char* const trash = smem_ring + NBUF * bufB;
    const int ch_begin = blockIdx.z * a.per_split;
    const int ch_end = min(a.nchunk, ch_begin + a.per_split);
    const __amdgpu_buffer_rsrc_t dr = __builtin_amdgcn_make_buffer_rsrc(
        uni_ptr(a.dense), (short)0, uni(a.B * a.M * HQ * EB), 0x00020000);
    const __amdgpu_buffer_rsrc_t gr = __builtin_amdgcn_make_buffer_rsrc(
        uni_ptr(a.gath), (short)0, uni(a.B * a.C * a.Hg * a.Wg * EB), 0x00020000);

    // chunk-invariant slot offsets (elements): Dense row m's position run, window piece (channel, row, column)
    int doff[ND], goff[NG], grow[NG], gcol[NG];
#pragma unroll
    for (int j = 0; j < ND; ++j) {
        const int gi = wave + j * NW;
        const int row = gi * RPI + lane / PPR;
        const int ql = ((lane % PPR) ^ lp_swz<PPR>(row)) * PE;
        const int m = m0 + row;
        doff[j] = (gi < NDG && m < a.M) ? m * HQ + (ql / a.cols) * a.Wq + ql % a.cols : -1;
    }
    const int wqp = a.wca >> LPE, pq = a.pitch_c >> LPE, npiece = kLC * pq;
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        const int pc = (wave + j * NW) * 64 + lane;
        const int cl = pc / pq, rem = pc - (pc / pq) * pq;
        const int wrow = rem / wqp, wx = (rem - wrow * wqp) * PE;
        const bool ok = pc < npiece && c0 + cl < a.C && wrow < a.wr;
        goff[j] = ((c0 + cl) * a.Hg + wrow) * a.Wg + wx;
        grow[j] = ok ? wrow : -(1 << 20);   // (an invalid piece fails the row test of every chunk)
        gcol[j] = wx;
    }

    auto issue = [&](int buf, int b, int qy0, int qx0) {
        char* base = smem_ring + buf * bufB;
        const int dbase = b * a.M * HQ + qy0 * a.Wq + qx0;
#pragma unroll
        for (int j = 0; j < ND; ++j) {
            const int gi = wave + j * NW;
            const int voff = doff[j] >= 0 ? (dbase + doff[j]) * EB : kOOB;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(dr, (lds_ptr_t)(gi < NDG ? base + gi * 1024 : trash), 16, voff, 0, 0, 0);
        }
        const int row0 = qy0 * S - 1, colA = qx0 * S - PE;   // pad 1, e = PE - 1
        const int gbase = (b * a.C * a.Hg + row0) * a.Wg + colA;
#pragma unroll
        for (int j = 0; j < NG; ++j) {
            const int gi = wave + j * NW;
            const bool ok = (unsigned)(row0 + grow[j]) < (unsigned)a.Hg && (unsigned)(colA + gcol[j]) < (unsigned)a.Wg;
            const int voff = ok ? (gbase + goff[j]) * EB : kOOB;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(gr, (lds_ptr_t)(gi * 64 < npiece ? base + BM * QC * EB + gi * 1024 : trash),
                                                     16, voff, 0, 0, 0);
        }
    };

    floatx16 acc[MF][KK];
    clear_acc(acc);

    // per-lane byte offsets inside a buffer for k-step ks: the A pieces of fragment f, the window run start
    int aoff[NKS][MF][NA], boff[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        const int q0 = ks * 16 + 8 * h;
        const int rl = q0 / a.cols, xl0 = q0 - rl * a.cols;
#pragma unroll
        for (int f = 0; f < MF; ++f) {
            const int row = (wm * MF + f) * 32 + r;
#pragma unroll
            for (int u = 0; u < NA; ++u) aoff[ks][f][u] = row * QC * EB + ((((q0 >> LPE) + u) ^ lp_swz<PPR>(row)) << 4);
        }
        boff[ks] = BM * QC * EB + (r * a.pitch_c + (rl * S + ky) * a.wca + xl0 * S) * EB;
    }

    // the issue cursor (chunk ch_begin + k, walked without divisions): sample, chunk row / column origin
    int ib, iqy, iqx;
    chunk_origin(a, QC, ch_begin, ib, iqy, iqx);
    auto advance = [&]() {
        iqx += a.cols;
        if (iqx >= a.Wq) {
            iqx = 0, iqy += a.rows;
            if (iqy >= a.Hq) iqy = 0, ++ib;
        }
    };
    const int n = ch_end - ch_begin;
#pragma unroll
    for (int k = 0; k < NBUF - 1; ++k)
        if (k < n) issue(k, ib, iqy, iqx), advance();
    int buf = 0, ibuf = NBUF - 1;   // ibuf = (k + NBUF - 1) % NBUF: chunk k - 1's buffer
    for (int k = 0; k < n; ++k) {
        // outstanding: chunks k .. k + ahead; chunk k must land, the ahead younger ones may stay in flight
        const int ahead = min(n - 1 - k, NBUF - 2);
        if constexpr (NBUF == 3) {
            if (ahead >= 1) lp_wait_vm_barrier<NL>(); else lp_wait_vm_barrier<0>();
        } else {
            if (ahead >= 2) lp_wait_vm_barrier<2 * NL>(); else if (ahead == 1) lp_wait_vm_barrier<NL>(); else lp_wait_vm_barrier<0>();
        }
        // chunk k landed for every wave; every wave is done with chunk k - 1's buffer: refill it
        if (k + NBUF - 1 < n) {
            issue(ibuf, ib, iqy, iqx);
            advance();
        }
        ibuf = ibuf + 1 == NBUF ? 0 : ibuf + 1;
        const char* sb = smem_ring + buf * bufB;
        buf = buf + 1 == NBUF ? 0 : buf + 1;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            u32x4 ra[MF][NA], rb[NB];
#pragma unroll
            for (int f = 0; f < MF; ++f)
#pragma unroll
                for (int u = 0; u < NA; ++u) ra[f][u] = lp_lds_read(sb + aoff[ks][f][u]);
#pragma unroll
            for (int i = 0; i < NB; ++i) rb[i] = lp_lds_read(sb + boff[ks] + 16 * i);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int f = 0; f < MF; ++f)
#pragma unroll
                for (int u = 0; u < NA; ++u) asm volatile("" : "+v"(ra[f][u]));
#pragma unroll
            for (int i = 0; i < NB; ++i) asm volatile("" : "+v"(rb[i]));
            decltype(lp_dense_frag<EB>(ra[0])) fa[MF];
#pragma unroll
            for (int f = 0; f < MF; ++f) fa[f] = lp_dense_frag<EB>(ra[f]);
            unsigned w[4 * NB];
#pragma unroll
            for (int i = 0; i < NB; ++i) w[4 * i + 0] = rb[i][0], w[4 * i + 1] = rb[i][1], w[4 * i + 2] = rb[i][2], w[4 * i + 3] = rb[i][3];
            static_for<0, KK>([&](auto kxc) {
                constexpr int kx = decltype(kxc)::value;
                const auto fb = lp_cut<EB, S, kx>(w);
#pragma unroll
                for (int f = 0; f < MF; ++f) acc[f][kx] = mma32x16<DT>(fa[f], fb, acc[f][kx]);
            });
        }
    }
    lp_store_partial<KK, MF>(a, acc, m0 + wm * MF * 32, c0 + r, ky, h);
}

struct LpPlan {
    int S, KK, BM, WM, QC, splits, lds_bytes;
    int eb;      // bytes per element of the LDS tiles (a holds that geometry): 4, or 2 on the ring of 16-bit maps
    int nbuf;    // 2: wgrad_staged_kernel; 3 / 4: wgrad_ring_kernel's depth
    LpArgs a;
};

// LDM_WGRAD_RING = 2 / 3 / 4 (default 3: a train step of 3.279-3.282 ms against 3.288-3.304 with 4): the ring's
// depth; 2 = no ring, the staged form
static int lp_ring_depth() {
    static const int ring = [] {
        const char* e = std::getenv("LDM_WGRAD_RING");
        const int v = e ? (int)std::strtol(e, nullptr, 0) : 3;
        return v < 2 ? 2 : (v > 4 ? 4 : v);
    }();
    return ring;
}

// Double-rate form: pad 1, k 3 / 4, stride 1 / 2, rows of 16 or a multiple of 32 positions, C >= 16.  st16: bit 0
// Dense, bit 1 Gath stored in 16 bits.  Both maps of one width whose rows split into whole pieces take the ring at
// that width, as deep as LDM_WGRAD_RING asks and the LDS holds; everything else the staged form.  K is split
// over blocks until the grid covers the 256 CUs (one block per CU: the buffers take 60-150 KB of LDS); the
// split does not depend on st16, so the workspace query (wgrad2_plan_ws) plans with any.
bool lp_plan(const ldm_conv_desc& d, int st16, LpPlan& p) {
    if (d.kh != d.kw || (d.kh != 3 && d.kh != 4) || (d.stride != 1 && d.stride != 2) || d.pad != 1) return false;
    LpArgs a{};
    conv_dims(d, a);
    if (a.C < 16 || a.Wg % 4) return false;
    int qc = 32;
    if (a.Wq % 32 == 0) {
        a.cols = 32, a.rows = 1;
    } else if (a.Wq == 16 && a.Hq % 2 == 0) {
        a.cols = 16, a.rows = 2;
    } else if (a.Wq == 16) {
        qc = 16, a.cols = 16, a.rows = 1;
    } else if (a.Wq == 8 && a.Hq % 2 == 0) {
        qc = 16, a.cols = 8, a.rows = 2;
    } else {
        return false;
    }
    const int S = d.stride, KK = d.kh;
    p.S = S, p.KK = KK, p.QC = qc;
    p.BM = a.M >= 128 ? 128 : (a.M > 32 ? 64 : 32);
    p.WM = p.BM == 128 ? 2 : 1;
    a.cps = a.Hq * a.Wq / qc;
    a.nchunk = a.B * a.cps;
    a.wr = (a.rows - 1) * S + KK;
    p.eb = st16 == 3 ? 2 : 4;
    p.nbuf = (st16 == 0 || (st16 == 3 && a.Wg % 8 == 0)) ? lp_ring_depth() : 2;
    while (p.nbuf > 2 && lp_lds_bytes(p.eb, p.nbuf, p.BM, qc, lp_pitch(p.eb, S, KK, a.rows, a.cols)) > kLdsMax) --p.nbuf;
    if (p.nbuf == 2) p.eb = 4;   // the staged form's tiles are floats
    a.wca = lp_wca(p.eb, S, KK, a.cols);
    a.pitch_c = lp_pitch(p.eb, S, KK, a.rows, a.cols);
    p.lds_bytes = lp_lds_bytes(p.eb, p.nbuf, p.BM, qc, a.pitch_c);
    if (p.lds_bytes > kLdsMax) return false;
    const int tiles = ((a.M + p.BM - 1) / p.BM) * ((a.C + kLC - 1) / kLC);
    static const int smax = [] {   // LDM_WGRAD_SPLITS: the largest K split (A/B timing; default 256)
        const char* e = std::getenv("LDM_WGRAD_SPLITS");
        const int v = e ? (int)std::strtol(e, nullptr, 0) : 256;
        return v < 1 ? 1 : (v > 256 ? 256 : v);
    }();
    int s = 1;
    while (s < smax && tiles * s < 256 && a.nchunk / (s * 2) >= 4) s *= 2;
    p.splits = s;
    a.per_split = (a.nchunk + s - 1) / s;
    p.a = a;
    return true;
}

template <int S, int KK, int BM, int WM, int QC, int DT, int EB, int NBUF>
int launch_ring(const LpPlan& p, hipStream_t st) {
    constexpr int NW = WM * KK;
    // the slot counts the kernel assumes cover this plan's pieces (its window groups fit NG slots per wave)
    LDM_REQUIRE((kLC * (p.a.pitch_c / (16 / EB)) + 63) / 64 <= lp_slots(EB, S, KK, QC, NW) * NW, "wgrad ring: window slots");
    LDM_REQUIRE(p.a.cols * p.a.rows == QC, "wgrad ring: chunk geometry");
    const dim3 grid((p.a.C + kLC - 1) / kLC, (p.a.M + BM - 1) / BM, p.splits);
    return launch_lds<wgrad_ring_kernel<S, KK, BM, WM, QC, DT, EB, NBUF>>("wgrad_ring_kernel", grid, 64 * NW, p.lds_bytes, st, p.a);
}
template <int S, int KK, int BM, int WM, int QC, int DT>
int launch_staged(const LpPlan& p, hipStream_t st) {
    constexpr int NW = WM * KK;
    // holds by construction: lp_slots takes the larger of the two geometries lp_plan makes for a QC
    LDM_REQUIRE((kLC * (p.a.pitch_c / 4) + 64 * NW - 1) / (64 * NW) <= lp_slots(4, S, KK, QC, NW), "wgrad staged: window slots");
    LDM_REQUIRE(p.a.cols * p.a.rows == QC, "wgrad staged: chunk geometry");
    const dim3 grid((p.a.C + kLC - 1) / kLC, (p.a.M + BM - 1) / BM, p.splits);
    return launch_lds<wgrad_staged_kernel<S, KK, BM, WM, QC, DT>>("wgrad_staged_kernel", grid, 64 * NW, p.lds_bytes, st, p.a);
}
template <int S, int KK, int BM, int WM, int QC, int DT>
int launch_lp_dt(const LpPlan& p, hipStream_t st) {
    if (p.nbuf == 2) return launch_staged<S, KK, BM, WM, QC, DT>(p, st);
    if (p.eb == 2)
        return p.nbuf == 4 ? launch_ring<S, KK, BM, WM, QC, DT, 2, 4>(p, st) : launch_ring<S, KK, BM, WM, QC, DT, 2, 3>(p, st);
    return p.nbuf == 4 ? launch_ring<S, KK, BM, WM, QC, DT, 4, 4>(p, st) : launch_ring<S, KK, BM, WM, QC, DT, 4, 3>(p, st);
}
template <int S, int KK, int QC, int DT>
int launch_lp_bm(const LpPlan& p, hipStream_t st) {
    switch (p.BM) {
        case 128: return launch_lp_dt<S, KK, 128, 2, QC, DT>(p, st);
        case 64: return launch_lp_dt<S, KK, 64, 1, QC, DT>(p, st);
        default: return launch_lp_dt<S, KK, 32, 1, QC, DT>(p, st);
    }
}
template <int S, int KK, int DT>
int launch_lp_qc(const LpPlan& p, hipStream_t st) {
    return p.QC == 16 ? launch_lp_bm<S, KK, 16, DT>(p, st) : launch_lp_bm<S, KK, 32, DT>(p, st);
}
template <int DT>
int launch_lp(const LpPlan& p, hipStream_t st) {
    switch (p.S * 10 + p.KK) {
        case 13: return launch_lp_qc<1, 3, DT>(p, st);
        case 23: return launch_lp_qc<2, 3, DT>(p, st);
        case 14: return launch_lp_qc<1, 4, DT>(p, st);
        default: return launch_lp_qc<2, 4, DT>(p, st);
    }
}

struct Plan {
    int S, KK, BM, BC, splits;
    Args a;
    int lds_bytes;
};

// Geometry and instance choice; false when this form does not apply (the caller keeps backward.hip's).
bool plan(const ldm_conv_desc& d, Plan& p) {
    if (d.kh != d.kw || (d.kh != 3 && d.kh != 4) || (d.stride != 1 && d.stride != 2) || d.pad < 0 || d.pad > 3)
        return false;
    Args a{};
    conv_dims(d, a);
    a.pad = d.pad;
    if (a.Wq % 4 || a.Wg % 4) return false;
    if (a.Wq >= kKQ ? (a.Wq % kKQ != 0) : (kKQ % a.Wq != 0)) return false;
    a.cols = a.Wq >= kKQ ? kKQ : a.Wq;
    a.rows = kKQ / a.cols;
    if (a.rows > a.Hq) a.rows = a.Hq;   // a small image: one chunk per sample, the rest zero-padded
    a.cps = a.Wq >= kKQ ? a.Hq * (a.Wq / kKQ) : (a.Hq + a.rows - 1) / a.rows;
    a.nchunk = a.B * a.cps;
    const int KK = d.kh, S = d.stride;
    a.e = ((a.pad % 4) == 0) ? 0 : 4 - (a.pad % 4);          // origin qx0*S - pad, qx0*S a multiple of 4
    a.wr = (a.rows - 1) * S + KK;
    const int wc = (a.cols - 1) * S + KK;
    a.wca = (a.e + wc + 3) / 4 * 4;
    a.pitch_c = a.wr * a.wca;
    p.S = S, p.KK = KK;
    p.BC = a.C == 1 ? 1 : (a.C <= 16 || KK == 4) ? 16 : 32;
    p.BM = (p.BC == 32 && a.M <= 32) ? 32 : 64;
    p.lds_bytes = 2 * buf_floats(p.BM * kKQ, p.BC, a.pitch_c) * 4;
    if (p.lds_bytes > kLdsMax) return false;
    const int tiles = ((a.M + p.BM - 1) / p.BM) * ((a.C + p.BC - 1) / p.BC);
    // the one-channel kernel keeps 4 blocks per CU resident: up to 1024 splits
    const int smax = p.BC == 1 ? 1024 : 256, want = p.BC == 1 ? 1024 : 512;
    int s = 1;
    while (s < smax && tiles * s < want && a.nchunk / (s * 2) >= 2) s *= 2;
    p.splits = s;
    a.per_split = (a.nchunk + s - 1) / s;
    p.a = a;
    return true;
}

template <int S, int KK, int BM, int BC, int DT>
int launch_dt(const Plan& p, hipStream_t st) {
    const dim3 grid((p.a.C + BC - 1) / BC, (p.a.M + BM - 1) / BM, p.splits);
    return launch_lds<wgrad_kernel<S, KK, BM, BC, DT>>("wgrad_kernel (tap-shared)", grid, 256, p.lds_bytes, st, p.a);
}

template <int S, int KK, int DT>
int launch_c1_dt(const Plan& p, hipStream_t st) {
    const dim3 grid(1, (p.a.M + 63) / 64, p.splits);
    if (DT != 0 && p.a.dense16)
        return launch_lds<wgrad_c1_kernel<S, KK, DT, DT>>("wgrad_c1_kernel", grid, 256, p.lds_bytes, st, p.a);
    return launch_lds<wgrad_c1_kernel<S, KK, DT, 0>>("wgrad_c1_kernel", grid, 256, p.lds_bytes, st, p.a);
}
template <int S, int KK>
int launch_c1(const Plan& p, hipStream_t st) {
    switch (p.a.lowp) {
        case LDM_DT_F32: return launch_c1_dt<S, KK, 0>(p, st);
        case LDM_DT_F16: return launch_c1_dt<S, KK, 1>(p, st);
        default: return launch_c1_dt<S, KK, 2>(p, st);
    }
}

template <int S, int KK, int BM, int BC>
int launch(const Plan& p, hipStream_t st) {
    switch (p.a.lowp) {
        case LDM_DT_F32: return launch_dt<S, KK, BM, BC, 0>(p, st);
        case LDM_DT_F16: return launch_dt<S, KK, BM, BC, 1>(p, st);
        default: return launch_dt<S, KK, BM, BC, 2>(p, st);
    }
}

}  // namespace wg

// LDM_WGRAD_LP=0 in the environment keeps 16-bit weight gradients on the tap-shared kernel (A/B timing
// and the parity test of both forms).
static bool wgrad_lp_disabled() {
    const char* e = getenv("LDM_WGRAD_LP");
    return e && e[0] == '0';
}

bool wgrad2_plan_ws(const ldm_conv_desc& d, int64_t& ws_floats) {
    wg::Plan p;
    if (!wg::plan(d, p)) return false;
    ws_floats = (int64_t)p.splits * p.a.M * p.a.C * p.KK * p.KK;
    wg::LpPlan lp;
    if (wg::lp_plan(d, 0, lp)) ws_floats = std::max(ws_floats, (int64_t)lp.splits * lp.a.M * lp.a.C * lp.KK * lp.KK);
    return true;
}

// Which tensors of the weight gradient of d may be stored in 16 bits (LDM_DT_X16 | LDM_DT_DY16) at a 16-bit
// operand precision: the double-rate form takes both (either or both: the staged kernel, both: the ring), the
// one-channel kernel (Cin = 1 layers) a 16-bit Dense (dy of a conv); else none.
int wgrad2_storage16(const ldm_conv_desc& d) {
    wg::Plan p;
    if (!wg::plan(d, p)) return 0;
    wg::LpPlan lp;
    if (!wgrad_lp_disabled() && wg::lp_plan(d, 3, lp)) return LDM_DT_X16 | LDM_DT_DY16;
    if (p.BC == 1) return d.transposed ? LDM_DT_X16 : LDM_DT_DY16;
    return 0;
}

// Runs the weight gradient into `partial` ([splits][M][N]); returns the split count through `splits`, or -1 when
// no form of this file applies.  st16: bit 0 Dense, bit 1 Gath stored in 16 bits (-2: not on this layer's forms)
int wgrad2_run(const ldm_conv_desc& d, const float* dense, const float* gath, float* partial, int& splits, int dtype,
               hipStream_t st, int st16, float* dw_direct) {
    wg::Plan p;
    if (!wg::plan(d, p)) return -1;
    if (dtype != LDM_DT_F32 && !wgrad_lp_disabled()) {   // 16-bit operands: the double-rate MFMA form
        wg::LpPlan lp;
        if (wg::lp_plan(d, st16, lp)) {
            lp.a.dense = dense;
            lp.a.gath = gath;
            lp.a.partial = partial;
            lp.a.dense16 = st16 & 1;
            lp.a.gath16 = (st16 >> 1) & 1;
            splits = lp.splits;
            if (lp.splits == 1 && dw_direct) {   // one K range: its partial is the gradient (no reduce launch)
                lp.a.partial = dw_direct;
                splits = 0;
            }
            return dtype == LDM_DT_F16 ? wg::launch_lp<1>(lp, st) : wg::launch_lp<2>(lp, st);
        }
    }
    if (st16 && (p.BC != 1 || (st16 & 2) || dtype == LDM_DT_F32)) return -2;
    p.a.dense16 = st16 & 1;
    p.a.lowp = dtype;
    p.a.dense = dense;
    p.a.gath = gath;
    p.a.partial = partial;
    splits = p.splits;
    if (p.BC == 1) {
        switch (p.S * 10 + p.KK) {
            case 13: return wg::launch_c1<1, 3>(p, st);
            case 23: return wg::launch_c1<2, 3>(p, st);
            case 14: return wg::launch_c1<1, 4>(p, st);
            case 24: return wg::launch_c1<2, 4>(p, st);
            default: return -1;
        }
    }
    const int key = p.S * 1000 + p.KK * 100 + (p.BM == 64 ? 10 : 0) + (p.BC == 32 ? 1 : 0);
    switch (key) {
        case 1311: return wg::launch<1, 3, 64, 32>(p, st);
        case 1301: return wg::launch<1, 3, 32, 32>(p, st);
        case 1310: return wg::launch<1, 3, 64, 16>(p, st);
        case 2311: return wg::launch<2, 3, 64, 32>(p, st);
        case 2301: return wg::launch<2, 3, 32, 32>(p, st);
        case 2310: return wg::launch<2, 3, 64, 16>(p, st);
        case 2410: return wg::launch<2, 4, 64, 16>(p, st);
        case 1410: return wg::launch<1, 4, 64, 16>(p, st);
        default: return -1;
    }
}

}  // namespace ldm
