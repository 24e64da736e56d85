/*
 * ldm_capi.h — C ABI of the MI355X-native latent-diffusion hot path (libldm_amd.so).
 *
 * The reference (PrioteasaAndrei/music-style-transfer-ldm) has no native boundary: its hot path is
 * nn.Module.__call__ -> ATen.  This header is the thin C ABI the drop-in Python
 * modules (music-style-transfer-ldm_amd/models/ (*.py)) call through ctypes.  Each entry point names the
 * reference code it replaces.
 *
 * Conventions
 *   - Plain pointers + sizes; every tensor is a contiguous fp32 NCHW device buffer unless stated.
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream); every
 *     launch goes on it, nothing is synchronised, nothing is allocated: workspaces come from the
 *     caller (graph-capture safe, §8(b) "Ownership").
 *   - Return 0 on success, otherwise a nonzero code; ldm_last_error() gives the message
 *     (thread-local).  The Python layer raises RuntimeError with it.
 */
#ifndef LDM_CAPI_H
#define LDM_CAPI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDM_CAPI_VERSION 1

/* ---- errors / introspection --------------------------------------------------------------- */
const char* ldm_last_error(void);
int ldm_capi_version(void);
/* Number of HIP devices visible to the runtime this library is bound to (no kernel launch). */
int ldm_device_count(int* count);

/* ---- 2-D convolution / transposed convolution -----------------------------------------------
 * Replaces nn.Conv2d / nn.ConvTranspose2d (+ following BatchNorm2d(eval) / ReLU / Tanh / time-emb
 * add / skip add) at model.py:16-25 (encoder), :37-46 (decoder), :61-79 (style encoder),
 * :178-194 + :205-229 (UNet).  Implicit GEMM on f32 MFMA (v_mfma_f32_32x32x2_f32 /
 * v_mfma_f32_16x16x4_f32), transposed convs as sub-pixel phases, fused epilogue. */
typedef struct ldm_conv_desc {
    int32_t B, Cin, Hin, Win;
    int32_t Cout, Hout, Wout;
    int32_t kh, kw, stride, pad, out_pad;
    int32_t transposed; /* 0: Conv2d weight [Cout,Cin,kh,kw]; 1: ConvTranspose2d weight [Cin,Cout,kh,kw] */
    int32_t layout;     /* activation layouts: bit 0 input NHWC, bit 1 output (and skip) NHWC; 0 = NCHW  */
} ldm_conv_desc;

enum {
    LDM_ACT_NONE = 0,
    LDM_ACT_RELU = 1,
    LDM_ACT_TANH = 2,
    LDM_ACT_TANH_HALF = 3, /* (tanh(x)+1)/2: decoder output rescale, model.py:371,:405,:498 */
    LDM_ACT_GELU = 4       /* exact erf GELU (nn.GELU(), model.py:173)                     */
};

/* Operand precision of the MFMA kernels: fp32 operands (exact), or rounded to fp16 / bf16 in registers
 * with fp32 accumulation, fp32 epilogue and fp32 outputs / sampler state (the torch.autocast fp16 / bf16
 * regions of the train step and of a sampling loop; BASELINE configs 3 and 5). */
enum { LDM_DT_F32 = 0, LDM_DT_F16 = 1, LDM_DT_BF16 = 2 };
/* Or'ed into ldm_epilogue.dtype (with LDM_DT_F16 / LDM_DT_BF16): ATen's autocast OUTPUT semantics as well —
 * the conv output, the eval-BN output, the activation and each add are rounded to that type (stored in the
 * fp32 tensor), as the reference's conv / linear outputs are 16-bit tensors inside torch.autocast
 * (train.py:174).  Or'ed into the act code of ldm_batchnorm_train_out / ldm_batchnorm_apply_out as
 * LDM_ACT_ROUND_F16 / LDM_ACT_ROUND_BF16: the BatchNorm output likewise (a 16-bit input's BN output). */
enum { LDM_DT_ROUND_OUT = 0x100 };
enum { LDM_ACT_ROUND_F16 = LDM_DT_F16 << 8, LDM_ACT_ROUND_BF16 = LDM_DT_BF16 << 8 };
/* 16-bit storage of the train step's large maps (ATen keeps the outputs of an autocast region in fp16 / bf16):
 *  - conv entry points, or'ed into ldm_epilogue.dtype with LDM_DT_F16 / _BF16: the input x (LDM_DT_X16), the
 *    output y and act_out (LDM_DT_Y16) are stored in that type; ldm_conv_backward_weight_dt's dtype takes
 *    LDM_DT_X16 (x) and LDM_DT_DY16 (dy);
 *  - BatchNorm / activation-backward entry points: bits 16-17 of the act code name the 16-bit type
 *    (LDM_DT_F16 / _BF16 << LDM_ST_SHIFT), and LDM_ST_* which of the call's tensors are stored in it: X16 the
 *    BatchNorm input x (activation backward: act_out), Y16 the BatchNorm output y, DY16 the incoming gradient,
 *    DX16 the outgoing gradient (dx / dv).  The pointers stay typed float* in the signatures. */
enum { LDM_DT_X16 = 0x200, LDM_DT_Y16 = 0x400, LDM_DT_DY16 = 0x800 };
enum { LDM_ST_SHIFT = 16, LDM_ST_X16 = 1 << 18, LDM_ST_Y16 = 1 << 19, LDM_ST_DY16 = 1 << 20, LDM_ST_DX16 = 1 << 21 };

typedef struct ldm_epilogue {
    const float* bias;      /* [Cout] or NULL                                                */
    const float* bn_weight; /* eval-mode BatchNorm2d after bias (NULL = none): gamma [Cout]    */
    const float* bn_bias;   /*   beta [Cout]                                                   */
    const float* bn_mean;   /*   running_mean [Cout]                                           */
    const float* bn_var;    /*   running_var [Cout]                                            */
    float bn_eps;
    int32_t act;            /* LDM_ACT_*                                                       */
    const float* bcast_add; /* [B,Cout] added after act (UNet time embedding, model.py:206)   */
    const float* skip_add;  /* [B,Cout,Hout,Wout] added after act (UNet skips, model.py:221) */
    float* act_out;         /* [B,Cout,Hout,Wout] or NULL: also store act(.) before the adds  */
                            /* (training: the activation's backward needs it)                */
    int32_t dtype;          /* operand precision LDM_DT_* of the conv kernels: fp32, or x and w rounded */
                            /* to fp16 / bf16 with fp32 accumulation (autocast); | LDM_DT_ROUND_OUT */
} ldm_epilogue;

typedef struct ldm_conv_plan {
    int32_t kind;          /* 0 direct (VALU), 1 MFMA 32x32x2 f32, 2 MFMA 16x16x4 f32, 3 LDS-staged */
                           /* 16-bit-operand MFMA 32x32x16 (tm = BM/64, tn = LDM_DT_F16 / _BF16),    */
                           /* 4 small-plane 16-bit-operand MFMA 32x32x16 (sconv.hip; tn = the dtype, */
                           /* wk = waves per block)                                                  */
    int32_t tm, tn, wk;    /* MFMA tiles per wave along M / N, waves splitting K per block      */
    int32_t ks;            /* blocks splitting K (>1: partial tiles + fixed-order last-arriver sum) */
    int32_t balance;       /* 4-phase transposed convs: phase p splits K ks*ntap_p ways (equal K per block) */
    int64_t packed_floats; /* size of the packed-weight buffer ldm_conv_pack_weight fills (0 = none) */
    int64_t ws_floats;     /* workspace floats the plan needs (ks > 1): tile counters, then partials */
} ldm_conv_plan;

int ldm_conv_make_plan(const ldm_conv_desc* d, ldm_conv_plan* plan);
/* The kind-3 plan for d at operand precision dtype (LDM_DT_F16 / LDM_DT_BF16): the LDS-staged implicit
 * GEMM for large-plane NCHW layers (Cin % 32 == 0, >= 4096 positions per phase; bias / eval-BN /
 * activation epilogues only).  Returns 0 and fills plan, or 1 when the layer is not of that class. */
int ldm_conv_tiled_plan(const ldm_conv_desc* d, int32_t dtype, ldm_conv_plan* plan);
/* The kind-4 plan for d at operand precision dtype (LDM_DT_F16 / LDM_DT_BF16): the small-plane implicit GEMM
 * (sconv.hip) for k3 p1 convs (stride 1 / 2) and k3 s2 op1 / stride-1 transposed convs whose phase grid tiles into
 * 32-position runs (Wq | 32, or Wq % 32 == 0), Cin % 32 == 0 (>= 64), Cout % 64 == 0, fp32 NCHW maps; every
 * epilogue but the position bias and the fused DDIM update.  Its weights use the kind-3 pack (ldm_conv_pack_weight).
 * Returns 0 and fills plan, or 1 when the layer is not of that class (LDM_AMD_SCONV=0: never). */
int ldm_conv_sconv_plan(const ldm_conv_desc* d, int32_t dtype, ldm_conv_plan* plan);
/* Force a specific plan (autotuning / tests).  Fills packed_floats / ws_floats; validates.
 * ks < 0 requests the phase-balanced split with base -ks (4-phase layers only). */
int ldm_conv_make_plan_forced(const ldm_conv_desc* d, int kind, int tm, int tn, int wk, int ks,
                              ldm_conv_plan* plan);
/* Re-lay the torch weight into the MFMA fragment order of `plan` (tap-major K, zero padded). */
int ldm_conv_pack_weight(const ldm_conv_desc* d, const ldm_conv_plan* plan, const float* w,
                         float* packed, void* stream);
/* y = epilogue(conv(x, w)).  `w` is the packed buffer for MFMA plans, the torch weight for direct.
 * Plans with ks > 1 need ldm_conv_forward_ws. */
/* The 16-bit storage flags (LDM_DT_X16 | LDM_DT_Y16) ldm_conv_forward takes for (d, plan) at a 16-bit operand
 * precision: both on kind-3 plans, a 16-bit output on the Cin = 1 stride-2 kernel, a 16-bit input on the
 * 64 -> 1 k4 s2 transposed conv; else 0. */
int32_t ldm_conv_storage16(const ldm_conv_desc* d, const ldm_conv_plan* plan);
int ldm_conv_forward(const ldm_conv_desc* d, const ldm_conv_plan* plan, const float* x, const float* w,
                     const ldm_epilogue* ep, float* y, void* stream);
/* The same with a caller-owned workspace of plan->ws_floats floats (may be NULL when that is 0).
 * Its leading counter words must be zero before the first call; every call leaves them zero again,
 * so one zero-initialised workspace serves any number of stream-ordered calls (not concurrent ones). */
int ldm_conv_forward_ws(const ldm_conv_desc* d, const ldm_conv_plan* plan, const float* x, const float* w,
                        const ldm_epilogue* ep, float* y, float* workspace, void* stream);

/* ---- BatchNorm2d, train mode (model.py:18,21,24,39,42 under .train(); model.py:307,344-347) ----
 * Batch statistics over (B,H,W) per channel, normalise in place, optional activation, and the
 * running-stat update (momentum, unbiased variance) exactly as nn.BatchNorm2d.  save_mean /
 * save_invstd [C] are written for the backward pass (may be NULL).  workspace:
 * ldm_reduce_workspace_floats(B,C,HW) floats, 8-byte aligned (reduce.hip).  Each channel is reduced
 * by a fixed set of slices in a fixed order (fp64 sums): bitwise reproducible. */
int64_t ldm_reduce_workspace_floats(int32_t B, int32_t C, int32_t HW);
int ldm_batchnorm_train(float* x, int32_t B, int32_t C, int32_t HW, const float* weight, const float* bias,
                        float* running_mean, float* running_var, float momentum, float eps, int32_t act,
                        float* save_mean, float* save_invstd, float* workspace, void* stream);
/* Out-of-place form (y may equal x): statistics of x, the normalised result into y.  The autograd path
 * uses it so that no copy of the input is made for the in-place kernel (functional.batchnorm). */
int ldm_batchnorm_train_out(const float* x, float* y, int32_t B, int32_t C, int32_t HW, const float* weight,
                            const float* bias, float* running_mean, float* running_var, float momentum, float eps,
                            int32_t act, float* save_mean, float* save_invstd, float* workspace, void* stream);
/* The same in two stages, for SyncBatchNorm (replaces torch.nn.SyncBatchNorm's batch_norm_stats /
 * batch_norm_gather_stats_with_counts / batch_norm_elemt for the data-parallel train path):
 * stats[2c] = sum x, stats[2c+1] = sum x^2 over this rank's batch (fp64) and stats[2C] = this rank's
 * B*H*W (stats holds 2C+1 doubles) -> the caller all-reduces all 2C+1 doubles over ranks (one collective;
 * the count rides along) -> apply.  apply's count > 0 is used as given; count <= 0 reads the global count
 * from stats[2C] on the device (no host synchronisation).  B may be 0 (an empty local shard joins the
 * all-reduce with zero sums and still updates the running statistics). */
int ldm_batchnorm_stats(const float* x, int32_t B, int32_t C, int32_t HW, double* stats, float* workspace,
                        void* stream);
/* ldm_batchnorm_stats with a storage code (LDM_ST_X16 | type << LDM_ST_SHIFT: a 16-bit input) */
int ldm_batchnorm_stats_code(const float* x, int32_t code, int32_t B, int32_t C, int32_t HW, double* stats,
                             float* workspace, void* stream);
int ldm_batchnorm_apply(float* x, int32_t B, int32_t C, int32_t HW, const double* stats, double count,
                        const float* weight, const float* bias, float* running_mean, float* running_var,
                        float momentum, float eps, int32_t act, float* save_mean, float* save_invstd, void* stream);
int ldm_batchnorm_apply_out(const float* x, float* y, int32_t B, int32_t C, int32_t HW, const double* stats,
                            double count, const float* weight, const float* bias, float* running_mean,
                            float* running_var, float momentum, float eps, int32_t act, float* save_mean,
                            float* save_invstd, void* stream);

/* ---- eval-mode BatchNorm2d (+activation) as a standalone op, out-of-place (y may equal x) ------ */
int ldm_batchnorm_eval(const float* x, float* y, int32_t B, int32_t C, int32_t HW, const float* weight,
                       const float* bias, const float* running_mean, const float* running_var, float eps, int32_t act,
                       void* stream);

/* ---- elementwise activation, out-of-place (y may equal x): ReLU / Tanh / (tanh+1)/2 / GELU ------ */
int ldm_activation(const float* x, float* y, int64_t n, int32_t act, void* stream);

/* ---- SinusoidalPositionEmbeddings.forward (model.py:239-246) alone: out [B,dim] ---------------- */
int ldm_sinusoid_embed(const void* t, int32_t t_is_float, int32_t B, int32_t dim, const float* freqs, float* out,
                       void* stream);

/* ---- time MLP: SinusoidalPositionEmbeddings -> Linear -> GELU -> Linear (model.py:170-175,
 * :239-246).  t: [B] int64 (t_is_float=0) or float32 (t_is_float=1); freqs [dim/2] = the
 * reference's exp(arange(half)*-(ln 1e4/(half-1))) table; w1,w2 [dim,dim] torch Linear layout. */
int ldm_time_mlp_forward(const void* t, int32_t t_is_float, int32_t B, int32_t dim, const float* freqs,
                         const float* w1, const float* b1, const float* w2, const float* b2, float* out,
                         void* stream);

/* ---- cross-attention core (nn.MultiheadAttention inside CrossAttention, model.py:126-160) -------
 * q [B,E,L] (the Q in-projection output in NCHW token order), kv [B,2E,S] (K channels then V
 * channels), out [B,E,L] = softmax((q*scale)^T k) v per head, written channel-major so the
 * out-projection reads it as NCHW (the reference's two permutes, model.py:144-158, vanish). */
/* Folded-query form for a fixed key set (the reverse loop's style maps): kf [B,heads,S,E] =
 * scale * Wq_h^T K_h, bf [B,heads,S] = scale * bq_h^T K_h from kv [B,2E,S] and the Q in-projection
 * (wq [E,E] torch layout, bq [E]); ldm_attention_folded then takes the projection's input z [B,L,E]
 * (token-major) and writes out [B,L,E] (token-major) = the same attention as q = Wq z + bq.
 * Replaces the Q in-projection + score product of nn.MultiheadAttention (model.py:153). */
int ldm_attention_fold_keys(const float* kv, const float* wq, const float* bq, int32_t B, int32_t E, int32_t heads,
                            int32_t S, float scale, float* kf, float* bf, void* stream);
int ldm_attention_folded(const float* z, const float* kv, const float* kf, const float* bf, float* out, int32_t B,
                         int32_t E, int32_t heads, int32_t L, int32_t S, void* stream);
/* Style mixing: the folded attention over any key count S >= 1 (several style references stacked along the keys)
 * with an optional additive key bias [B,S] (fp32; NULL = none; -inf removes a key, and a key run that is entirely
 * -inf contributes exactly 0):  out(q) = sum_s exp(q.k_s + bias_s) v_s / sum_s exp(q.k_s + bias_s).
 * Instances: E 256 and E 512 at 4 heads; any L >= 1.  S == L without a bias runs ldm_attention_folded; anything
 * else streams the keys in tiles with an online softmax (stylemix.hip).  z, kf and out 16-byte aligned.
 * ldm_attention_fold_keys_bias is ldm_attention_fold_keys with the bias added to bf (bf[b,h,s] += key_bias[b,s]),
 * so an attention that reads this bf needs no bias argument; key_bias NULL is ldm_attention_fold_keys itself. */
int ldm_attention_folded_keys(const float* z, const float* kv, const float* kf, const float* bf,
                              const float* key_bias, float* out, int32_t B, int32_t E, int32_t heads, int32_t L,
                              int32_t S, void* stream);
int ldm_attention_fold_keys_bias(const float* kv, const float* wq, const float* bq, int32_t B, int32_t E,
                                 int32_t heads, int32_t S, float scale, const float* key_bias, float* kf, float* bf,
                                 void* stream);
/* Style map: ldm_attention_folded_keys with a reference bias on top of the key bias.  The S keys are R references of
 * S / R keys each (S % R == 0; key s belongs to reference s / (S / R)), and ref_bias [Bm,L,R] (fp32, finite or -inf,
 * never NaN or +inf) is the log-weight of each reference at each QUERY position:
 *   out(q_l) = sum_s exp(q_l.k_s + bias_s + ref_bias[b][l][ref(s)]) v_s / (the same sum without v_s).
 * The softmax lane of (row l, key s) forms xb = (bf[s] (+ key_bias[s])) + ref_bias[b][l][ref(s)], then x = (score) + xb,
 * in that association, so a ref_bias that is constant over l gives bitwise what the same values give as a key bias.
 * Samples b >= Bm (0 <= Bm <= B) take no reference bias.  A row whose references are all -inf yields exactly 0.
 * ref_bias NULL is ldm_attention_folded_keys itself, bitwise.  Same instances (E 256 / 512, 4 heads), any L >= 1. */
int ldm_attention_folded_keys_map(const float* z, const float* kv, const float* kf, const float* bf,
                                  const float* key_bias, const float* ref_bias, int32_t R, int32_t Bm, float* out,
                                  int32_t B, int32_t E, int32_t heads, int32_t L, int32_t S, void* stream);
/* The folded attention's probabilities only: p [B,heads,L,S] = softmax(z^T kf_h + bf_h) (CA1's instance: E 512,
 * 4 heads, L, S <= 16).  The reverse loop's bottleneck then contracts them with its folded values (below). */
int ldm_attention_folded_probs(const float* z, const float* kf, const float* bf, float* p, int32_t B, int32_t E,
                               int32_t heads, int32_t L, int32_t S, void* stream);
/* The bottleneck after CA1 with the attention's values folded into its weights (bfold.hip; model.py:214-217):
 * u [B,512,576] = W' (x) V once per loop, u[b][co][(t*4 + h)*16 + s] = sum_d w_fold[co][h*128 + d][t] *
 * kv[b][512 + h*128 + d][s] (w_fold = the bottleneck o out-projection fold of ldm_fold_conv_proj, torch layout
 * [512,512,3,3]; kv the CA1 K/V projection [B,1024,16]); then per step y [B,2,8,512] (NHWC) = relu(sum over
 * (t, h, s) of u * p[b][h][l_t][s] + pos_bias[l][co]) with pos_bias [16][512] (position-major) and p from
 * ldm_attention_folded_probs.  dtype LDM_DT_F16 / _BF16 rounds the output to that type (operands stay fp32).
 * Used by ldm_sample when ldm_bneck_fold_supported(B, H, W): the canonical 16 x 64 latent, B <= 8
 * (LDM_BNECK_FOLD=0 turns it off). */
int32_t ldm_bneck_fold_supported(int32_t B, int32_t H, int32_t W);
int ldm_bneck_fold_values(const float* w_fold, const float* kv, float* u, int32_t B, void* stream);
int ldm_bneck_pv(const float* u, const float* p, const float* pos_bias, float* y, int32_t B, int32_t dtype,
                 void* stream);
/* CA1's probabilities P [B,4,16,16] only, one block of eight waves per (sample, head): the reverse loop's form
 * (LDM_CA1P_FORM=0 keeps ldm_attention_folded_probs).  z4 token-major [B,16,512], kf [B,4,16,512], bf [B,4,16]. */
int ldm_ca1_probs(const float* z4, const float* kf, const float* bf, float* p, int32_t B, void* stream);
/* The keys in MFMA fragment order for ldm_ca1_probs_packed (the loop's form): kf[b][h][s][e] goes to float index
 * (((((b*4 + h)*32 + e/16)*4 + (e%16)/4)*16 + s)*4 + e%4 of kf_packed (same size, a buffer of its own), i.e.
 * [b][h][e chunk of 16][lg = (e%16)/4][s][4 e]: a wave's 16-byte loads of one tile of 16 keys x 16 e are one
 * contiguous KB in lane order.  The same sums in the same order: p is bitwise ldm_ca1_probs' on the plain keys. */
int ldm_ca1_pack_keys(const float* kf, float* kf_packed, int32_t B, void* stream);
int ldm_ca1_probs_packed(const float* z4, const float* kf_packed, const float* bf, float* p, int32_t B, void* stream);
/* 1 when the reverse loop keeps CA1's keys packed and runs ldm_ca1_probs_packed (the default while
 * ldm_ca1_probs_form() is 1; LDM_BFOLD_PACKED=0 keeps the plain keys and ldm_ca1_probs, for A/B timing).  bench.py
 * --full's kernel table times ldm_ca1_probs on plain keys. */
int32_t ldm_bfold_packed_form(void);
/* 1 when the reverse loop forms CA1's probabilities with ldm_ca1_probs, 0 when with ldm_attention_folded_probs
 * (LDM_CA1P_FORM=0): what bench.py times for the loop's CA1 launch. */
int32_t ldm_ca1_probs_form(void);
/* A/B switch of the Cin = 1 stride-2 conv's packed form (two output channels per v_pk_fma_f32; bitwise the scalar
 * form's results): 1 on, 0 off; returns the previous setting.  Default: LDM_CIN1_PK. */
int ldm_set_cin1_packed(int on);
/* A/B switch of the Cin = 1 k3 stride-1 conv's four-column form (conv_cin1_x4_kernel, SD = 1: the UNet's first layer on
 * the raw mel, UNet(1, 1) at shape S; models/model.py:178 Conv2d(in_channels, num_filters, 3, 1, 1)) against the one-lane-per-pixel
 * kernel, bitwise the same results: 1 on, 0 off; returns the previous setting.  Default: LDM_CIN1_S1. */
int ldm_set_cin1_s1(int on);
/* A/B switch of the flash attention forward's key splits over blocks (flash.hip: where one block per (query tile,
 * head) fills under a quarter of the CUs — CA1 at shape S — the key tiles split over up to 4 blocks and a combine pass
 * merges their (O, m, l); CrossAttention, models/model.py:126-160): 1 on, 0 off; returns the previous setting.
 * Default: LDM_FLASH_SPLIT. */
int ldm_set_flash_split(int on);
/* A conv (descriptor d, weight w_conv [Cout,Cmid,kh,kw], bias b_conv or NULL) applied to the output of a
 * Linear/1x1 projection (w_proj [Cmid,Cin], b_proj [Cmid]) as ONE conv: w_out [Cout,Cin,kh,kw] =
 * w_conv o w_proj and pos_bias_out [Cout,Hout,Wout] = b_conv + the projection bias through the taps that
 * fall inside the input (padding taps see zeros).  Used for out_proj -> enc4 / bottleneck
 * (model.py:155-160 then :212 / :217) in the reverse loop. */
int ldm_fold_conv_proj(const ldm_conv_desc* d, const float* w_conv, const float* b_conv, const float* w_proj,
                       const float* b_proj, int32_t Cmid, float* w_out, float* pos_bias_out, void* stream);
int ldm_attention_core(const float* q, const float* kv, float* out, int32_t B, int32_t E, int32_t heads,
                       int32_t L, int32_t S, float scale, void* stream);
/* Width-general form (flash.hip; any L, S, head dim 64 or 128 — the UNet's token counts grow with the mel
 * width, model.py:140-153): KV-tiled online softmax, channel-major q / out as ldm_attention_core, plus
 * lse [B,heads,L] = the log-sum-exp of each query's scaled scores for ldm_attention_backward_flash.
 * ldm_attention_core itself hands over to this kernel when L or S exceeds its LDS-resident instances. */
int ldm_attention_flash_supported(int32_t E, int32_t heads);
int ldm_attention_forward_lse(const float* q, const float* kv, float* out, float* lse, int32_t B, int32_t E,
                              int32_t heads, int32_t L, int32_t S, float scale, void* stream);

/* ---- DDPM forward noising q_sample (ForwardDiffusion.forward, model.py:102-115) ----------------
 * z_t = sqrt(ab[t_b]) * x0 + sqrt(1-ab[t_b]) * eps.  coef_table [T,2] = {sqrt(ab), sqrt(1-ab)} per
 * timestep (device), t [B] int64 (device).  t outside [0,T) yields NaN for that sample (the
 * reference raises IndexError, model.py:107; the Python layer checks host-known t up front). */
int ldm_q_sample(const float* x0, const float* eps, const float* coef_table, int32_t T, const int64_t* t, float* zt,
                 int32_t B, int64_t per_sample, void* stream);
/* predict_start_from_noise (model.py:117-124): x0 = (z_t - sqrt(1-ab) * eps) / sqrt(ab), table as above. */
int ldm_predict_start(const float* zt, const float* eps, const float* coef_table, int32_t T, const int64_t* t,
                      float* x0, int32_t B, int64_t per_sample, void* stream);
/* Backward of the two gathers above: kind 0 (q_sample): grad_a = sqrt(ab)*g -> d x0, grad_b = sqrt(1-ab)*g
 * -> d eps; kind 1 (predict_start): grad_a = g/sqrt(ab) -> d z_t, grad_b = -sqrt(1-ab)*g/sqrt(ab) -> d eps.
 * Either output may be NULL. */
int ldm_sched_backward(int32_t kind, const float* grad, const float* coef_table, int32_t T, const int64_t* t,
                       float* grad_a, float* grad_b, int32_t B, int64_t per_sample, void* stream);
/* One reverse step of style_conditioned_ddim_sample / content_style_ddim_sample (model.py:439-463):
 * coef[4] = {sqrt(ab_t), sqrt(1-ab_t), sqrt(ab_next), sqrt(1-ab_next)} (device, uniform over the
 * batch), eta as in the reference (deterministic term).  x is updated in place; x0_log / eps_log
 * (may be NULL) receive pred_x0 / noise_pred clones.  Bitwise equal to the reference's fp32 op
 * sequence for identical inputs (no FMA contraction). */
int ldm_ddim_step(float* x, const float* eps, const float* coef, float eta, float* x0_log, float* eps_log,
                  int64_t n, void* stream);
/* One step of the multistep solver (DPM-Solver++ in its data-prediction form) on n elements, x in place:
 *   x0 = (x - sigma_t eps) / alpha_t;  x <- (c_x x + c_0 x0) + c_1 x0_prev,
 * fp32 with one rounding per operation.  coef: one row [8] {alpha_t, sigma_t, c_x, c_0, c_1, 0, 0, 0} of
 * ForwardDiffusion.multistep_coefs (device).  x0_prev: the previous step's x0, or NULL for a first-order step
 * (the term and its load are skipped).  x0_log (required, not x0_prev) receives x0; eps_log (or NULL) a copy
 * of eps. */
int ldm_msolver_step(float* x, const float* eps, const float* coef, const float* x0_prev, float* x0_log,
                     float* eps_log, int64_t n, void* stream);

/* ---- loss reductions (loss.py): kind 0 = mean((a-b)^2) (diffusion_loss :48-49, nn.MSELoss :35),
 * kind 1 = mean(0.5*(a^2-1-log(a^2+1e-8))) (kl_regularization_loss :31-32, b unused).
 * Deterministic: fixed partition, fp64 partials.  workspace >= 512 doubles; out is a device scalar. */
int ldm_loss_forward(int32_t kind, const float* a, const float* b, int64_t n, void* workspace, float* out,
                     void* stream);
/* grad_a / grad_b (may be NULL) = d(loss)/d(a|b) * grad_out[0] (device scalar). */
int ldm_loss_backward(int32_t kind, const float* a, const float* b, int64_t n, const float* grad_out, float* grad_a,
                      float* grad_b, void* stream);

/* ---- whole UNet forward (UNet.forward, model.py:196-231) and the DDIM sampling loop ------------- */
typedef struct ldm_unet_weights {
    /* conv layers in order enc1, enc2, enc3, enc4, bottleneck, dec4, dec3, dec2, dec1:
     * packed (or raw, for direct plans) weights and biases */
    const float* conv_w[9];
    const float* conv_b[9];
    ldm_conv_plan conv_plan[9];
    /* cross_attention2 (E=256) then cross_attention1 (E=512): packed Q-proj / KV-proj / out-proj */
    const float* ca_wq[2];
    const float* ca_bq[2];
    ldm_conv_plan ca_plan_q[2];
    const float* ca_wkv[2];
    const float* ca_bkv[2];
    ldm_conv_plan ca_plan_kv[2];
    const float* ca_wo[2];
    const float* ca_bo[2];
    ldm_conv_plan ca_plan_o[2];
    /* time MLP */
    const float* t_freqs;
    const float* t_w1;
    const float* t_b1;
    const float* t_w2;
    const float* t_b2;
    /* Re-associated forms used by the reverse loop when use_fold != 0 (ldm_fold_conv_proj,
     * ldm_attention_fold_keys): raw Q in-projection rows (in_proj_weight[:E], torch layout) of both
     * cross-attentions, and enc4 / bottleneck composed with the preceding out-projection
     * (packed with conv_plan[3] / conv_plan[4]) plus their position-dependent biases [Cout,Hout,Wout]. */
    const float* ca_wq_raw[2];
    const float* fold_w[2];
    const float* fold_pb[2];
    int32_t use_fold;
    /* Step kernels of the reverse loop (used when use_step != 0 together with use_fold, for latent C = 32
     * and num_filters = 64): the nine convs packed by ldm_step_pack_weight (enc4 / bottleneck: their
     * folded weights), and the folded position biases transposed to [Hout*Wout][Cout].  use_step 1: the
     * register-direct kernels (uconv.hip, any latent with H, W multiples of 8); 2: the same (it selected the
     * LDS-staged kernels of rounds 2-5, measured slower and removed in round 6). */
    const float* step_w[9];
    const float* step_pb[2];
    int32_t use_step;
    int32_t step_dtype;   /* LDM_DT_*: operand precision of the step kernels (not F32: uconv.hip only) */
    /* The bottleneck o CA1 out-projection fold in the torch layout [512,512,3,3] (ldm_fold_conv_proj's w_out,
     * unpacked): the source of the folded values U when the loop runs the bottleneck on them
     * (ldm_bneck_fold_supported; ldm_bneck_fold_values).  NULL: the uconv bottleneck. */
    const float* step_bneck_w;
} ldm_unet_weights;

typedef struct ldm_unet_shape {
    int32_t B, C, H, W;   /* latent [B,C,H,W]; style s5 [B,256,H/4,W/4], s6 [B,512,H/8,W/8] */
    int32_t nf;           /* num_filters (64)                                                   */
} ldm_unet_shape;

/* Workspace floats needed by ldm_unet_forward for this shape and these plans (w may be NULL: plans
 * without cross-block K splits).  The workspace must be zero-filled once before its first use (it
 * holds the split-K tile counters, which every call leaves zero again). */
int64_t ldm_unet_workspace_floats(const ldm_unet_shape* s, const ldm_unet_weights* w);
/* Fill the 9+6 conv plans of `w` for this shape (weights must then be packed by the caller). */
int ldm_unet_make_plans(const ldm_unet_shape* s, ldm_unet_weights* w);
/* Conv descriptors of the 9 convs + 6 projection GEMMs (index order as in ldm_unet_weights). */
int ldm_unet_layer_desc(const ldm_unet_shape* s, int32_t layer, ldm_conv_desc* d);
int ldm_unet_forward(const ldm_unet_shape* s, const ldm_unet_weights* w, const float* z, const void* t,
                     int32_t t_is_float, const float* s5, const float* s6, float* out, float* workspace,
                     void* stream);

/* ---- the reverse loop: one entry, its options in one struct ------------------------------------------------
 * Replaces style_conditioned_ddim_sample (model.py:409-465) / content_style_ddim_sample (:503-559).  x is updated in
 * place over nsteps = len(times)-1 steps.  The time MLP for all steps is one launch before the loop, the style
 * maps' K/V projections likewise, and each step's update is fused into dec1's epilogue.  Only launches: the caller
 * may capture the whole loop into one hipGraph (the Python layer does, with torch.cuda.CUDAGraph, splitting the
 * batch into independent sub-batch chains on separate streams so that one chain's launch / memory latency overlaps
 * another's work).  Every option is off when its fields are NULL / 0, and the options compose. */
#define LDM_SOLVER_DDIM 0        /* coef_table [nsteps,4] (ldm_ddim_step's rows), eta used, x0_logs optional */
#define LDM_SOLVER_MULTISTEP 1   /* coef_table [nsteps,8] (ldm_msolver_step's rows, ForwardDiffusion.multistep_coefs), */
                                 /* eta ignored, x0_logs required: the history (step i reads step i-1's slot)         */

typedef struct ldm_sample_args {
    int32_t solver, nsteps;   /* LDM_SOLVER_*; nsteps 0 returns at once */
    float eta;
    /* Style mixing: the loop attends over S5 / S6 style tokens per sample instead of the maps' own H*W/16 / H*W/64
     * (0 = the maps' own): s5 [B,256,S5], s6 [B,512,S6] (R references stacked along the map's height: reference r
     * owns keys [r*L, (r+1)*L)), key_bias5 [B,S5] / key_bias6 [B,S6] as in ldm_attention_folded_keys (log of each
     * reference's weight; NULL = none).  The K/V projections and the key fold run over S tokens, the bias is folded
     * into bf once per loop, and each step's two attentions stream the keys.  Other key counts or a bias need
     * use_fold (an error otherwise); with S6 != H*W/64 or a key_bias6 the bottleneck runs without its value fold. */
    int32_t S5, S6;
    /* Style map (refs 0 and both pointers NULL = none; the two pointers go together, one alone is an error): the
     * log-weight of each of the `refs` stacked references at every query position of the two cross-attentions,
     * ref_bias5 [B, H*W/16, refs] for CA2 and ref_bias6 [B, H*W/64, refs] for CA1 (fp32, finite or -inf; tokens
     * row-major as the UNet flattens its maps), as in ldm_attention_folded_keys_map.  S5 and S6 must be refs times the
     * maps' own counts (refs = 1: the maps' own, given as such or as 0).  Needs use_fold.  The biases add to the key
     * biases; with guidance they apply to the target half only (the base half runs unbiased); the bottleneck runs
     * without its value fold.  They are the caller's buffers, read by every step's two attentions in the run phase:
     * ldm_sample_prepare does not read them, and the workspace size does not depend on them. */
    int32_t refs;
    /* Joint sampling of overlapping windows (0 = off): batch rows b and b + 1 are neighbouring windows of one
     * recording that share seam_cols latent columns, 0 <= seam_cols <= W / 2 (another value is an error).  One seam
     * fuse replaces, for every b < B - 1, c, h and j in [0, seam_cols),
     *     a = x[b,c,h,W-seam_cols+j];  q = x[b+1,c,h,j];  w_j = (j + 1) / (seam_cols + 1);  m = a + w_j * (q - a)
     * (fp32, one rounding per operation: the division, d = q - a, p = w_j d, m = a + p) in both places by m.  The
     * loop fuses once before step 0 and after every step's update (after the keep blend when there is one): nsteps + 1
     * launches of one small kernel, and the returned x agrees bitwise across every seam.  The x0 / eps logs and the 2M
     * history stay each window's own prediction.  Guided, the target and the base half of the doubled state are fused
     * separately (no seam between them).  B == 1 is legal and launches nothing extra.  The rows of a joint loop are
     * not independent: a caller that splits a batch into chains must not split a joint one.  With 0 every entry
     * launches exactly what it launches without the field.  ldm_sample_prepare does not read the field, and the
     * workspace size does not depend on it. */
    int32_t seam_cols;
    float* x;                 /* [B,C,H,W], in place */
    const float *s5, *s6, *key_bias5, *key_bias6;
    const float *ref_bias5, *ref_bias6;
    /* Style guidance (all five NULL = none; s5_base, s6_base and guide_scale go together, the biases are optional):
     * every step evaluates the denoiser under the target maps (s5 / s6) and the base maps on the same x and t and
     * steps on
     *   eps = e_b + scale[b] * (e_t - e_b)      (fp32, one rounding per operation: d = e_t - e_b; g = s d; e = e_b + g)
     * with e_t / e_b dec1's outputs (after its output rounding with 16-bit operands); eps feeds the unchanged update,
     * the logs record the guided x0 / eps, and the multistep history is the guided x0.  scale = 1 is the unguided
     * sampler on the target up to one rounding, scale = 0 the one on the base.  The base maps and biases are
     * separate [B, ...] arrays with the target's key counts; guide_scale is a device array [B] of finite fp32.
     * s->B stays the caller's batch B, but the body runs the UNet at batch 2B (targets, then bases): w holds the
     * plans and weights bound for the shape with batch 2B (ldm_unet_make_plans on it).  One exception is allowed
     * with use_step: the plans may be those of a larger batch (a sub-batch chain running the whole batch's plans, so
     * that a sample's arithmetic does not depend on how a batch is split), provided the two K/V projection plans need
     * no split-K workspace (ws_floats == 0): a plan's kind, tile and weight pack do not depend on the batch, the grids
     * come from s, and those two projections are the step-kernel path's only planned launches.  Without use_step
     * dec1's bound plan must be of kind 0, 1 or 2 (what ldm_unet_make_plans produces); another kind is an error.
     * dec1 runs as two launches at batch B: the base half as a plain conv, the target half with the guidance and the
     * update fused, storing the new state for both halves. */
    const float *s5_base, *s6_base, *key_bias5_base, *key_bias6_base, *guide_scale;
    /* Regional keep (all four NULL = none; one NULL beside the others is an error): after every step's update the
     * state is blended with the content's own noising trajectory under a keep weight, per element in fp32, one
     * rounding per operation (keep_blend, csrc/common.h):
     *     known = a_i * z0 + b_i * n0;   x_next = (1 - w) * x_update + w * known
     * z0 / n0 [B,C,H,W]: the clean latent and the q_sample noise; keep [B,H,W] in [0,1] (1 = keep the content,
     * shared by the channels); keep_coef [nsteps,2] = {a_i, b_i} (device; ForwardDiffusion.keep_coefs).  The x0 /
     * eps logs and the 2M history stay the model's own prediction. */
    const float *z0, *n0, *keep, *keep_coef;
    const int64_t* t_table;   /* [nsteps,B]: times[i] repeated over the batch */
    const float* coef_table;  /* per-step coefficient rows of the solver */
    /* step i at x0_logs + i*log_step_stride ([B,C,H,W] each; stride 0 = dense B*C*H*W), so a sub-batch can write
     * straight into its slice of the full-batch logs; either may be NULL (x0_logs not for the multistep solver) */
    float *x0_logs, *eps_logs;
    int64_t log_step_stride;
    float* workspace;         /* ldm_sample_workspace_floats(s, w, this struct) floats, zero-filled before first use */
    void* stream;
} ldm_sample_args;

/* The workspace size of ldm_sample(s, w, a): size with the struct that will be passed.  Reads only nsteps, S5, S6
 * and whether the guidance / the keep are on (any pointer of the group set).  Negative for a NULL s or a, a
 * negative nsteps / S5 / S6 or a batch <= 0.  A guided workspace is more than twice the unguided one. */
int64_t ldm_sample_workspace_floats(const ldm_unet_shape* s, const ldm_unet_weights* w, const ldm_sample_args* a);
/* The struct carries no buffer size, so before anything is launched ldm_sample asks the runtime for the extent of the
 * device allocation that holds `workspace` and reports an error if it ends before ldm_sample_workspace_floats(s, w, a)
 * (a buffer sized for another configuration).  That is exact for a buffer that is an allocation of its own; one
 * carved out of a larger pool is only known to end inside the pool, and the check is skipped under stream capture
 * (run the loop eagerly once before capturing it). */
int ldm_sample(const ldm_unet_shape* s, const ldm_unet_weights* w, const ldm_sample_args* a);
/* ldm_sample in two phases, for callers that run many loops against one style (the windows of a recording, a sampler
 * service, a replayed graph).  Both take ldm_sample's arguments and make its checks.
 * ldm_sample_prepare launches what reads only the style maps (target and base), the key biases, t_table and the
 * weights: the time MLP over the whole t_table, the guided loop's doubled operands, the style maps' K/V projections,
 * both key folds and, where it applies, the bottleneck's value fold.  It reads neither x, the logs, coef_table,
 * guide_scale nor the keep operands, and leaves its results in regions of the workspace that no launch of the run
 * phase writes.
 * ldm_sample_run launches the rest (the state's layout in and out, the keep region's fill, the loop) on a workspace
 * that an ldm_sample_prepare with the same s, w and a — the same map, bias and table contents, key counts, nsteps and
 * weights — has filled since those last changed; any number of runs may follow one prepare, with other x, logs,
 * coef_table, eta, solver, guide_scale and keep operands, and with other reference biases (ref_bias5 / ref_bias6: the
 * prepare reads only whether they are set, never their contents, so one prepare serves every window of a recording
 * whatever its style map).  A run on a workspace prepared for other contents computes
 * with those: nothing detects it.
 * ldm_sample is ldm_sample_prepare then ldm_sample_run: the same launches in the same order, bitwise the same result.
 * All three make one set of argument checks, so that a struct one entry takes the others take too: ldm_sample_prepare
 * also wants x and coef_table (and x0_logs for the multistep solver) non-NULL although it reads none of them; a caller
 * that prepares before it has a state passes the buffers it will run with. */
int ldm_sample_prepare(const ldm_unet_shape* s, const ldm_unet_weights* w, const ldm_sample_args* a);
int ldm_sample_run(const ldm_unet_shape* s, const ldm_unet_weights* w, const ldm_sample_args* a);
/* The parts of the workspace that must be zero before a launch (they hold split-K tile counters, which every launch
 * leaves zero again): ranges[0..3] = {offset, length, offset, length} in floats, a length may be 0.  Every other
 * float of the workspace is written by ldm_sample_prepare or ldm_sample_run before it is read.  Reads what
 * ldm_sample_workspace_floats reads. */
int ldm_sample_workspace_zeroed(const ldm_unet_shape* s, const ldm_unet_weights* w, const ldm_sample_args* a,
                                int64_t* ranges);
/* The guidance and the keep arithmetic on whole tensors.  ldm_guide_eps: out[i] = e_b[i] + scale[i / per_sample] *
 * (e_t[i] - e_b[i]) for B * per_sample elements (out may alias e_t or e_b).  ldm_keep_blend: in place on x (NCHW),
 * with one row coef = {a, b}.  ldm_seam_fuse: one seam fuse of ldm_sample_args.seam_cols in place on x (NCHW),
 * 1 <= seam_cols <= W / 2; B == 1 launches nothing. */
int ldm_seam_fuse(float* x, int32_t B, int32_t C, int32_t H, int32_t W, int32_t seam_cols, void* stream);
int ldm_guide_eps(const float* e_t, const float* e_b, const float* scale, int64_t per_sample, int32_t B, float* out,
                  void* stream);
int ldm_keep_blend(float* x, const float* z0, const float* n0, const float* keep, const float* coef, int32_t B, int32_t C,
                   int64_t HW, void* stream);

/* ---- data formats either side of the path (dataio.hip) ---------------------------
 * ldm_mel_quantize: the reference's 8-bit mel PNG pixels, uint8(clip((db + max_db) * 255/max_db, 0, 255)
 * + 0.5) (audio_processor.py:55-73, fp32 arithmetic, bit-exact with its numpy); ldm_mel_dequantize: its
 * inverse db = u8 * max_db/255 - max_db (audio_processor.py:91-93); ldm_u8_to_unit: the [0,1] tensor the
 * model consumes, u8 / 255 (dataset.py:258, torchvision ToTensor). */
int ldm_mel_quantize(const float* db, uint8_t* out, int64_t n, float max_db, void* stream);
int ldm_mel_dequantize(const uint8_t* in, float* db, int64_t n, float max_db, void* stream);
int ldm_u8_to_unit(const uint8_t* in, float* out, int64_t n, void* stream);

/* ---- audio front and back end (audio.hip; DESIGN.md "Audio front and back end") ------------------------
 * librosa's defaults: periodic Hann window of n_fft points, hop = n_fft / 4, centre reflect padding.  Built for
 * n_fft 512 and 2048; everything fp32.  Complex arrays are interleaved (re, im) pairs; spectra are [B, F, T] with
 * F = n_fft/2 + 1 and T = 1 + L / hop frames (T contiguous).
 *
 * tables: the twiddle / window table of one n_fft on the device: ldm_stft_table_floats(n_fft) floats (0 for an
 * unsupported n_fft), filled on the host in float64 by ldm_stft_fill_tables and copied over by the caller.
 * ldm_stft: y [B, L] (L >= n_fft/2 + 1) -> S complex and / or mag = |S|^power (power 1 or 2); either may be null.
 * ldm_istft: y [B, L] = overlap-add of the inverse frames of S (times mag [B, F, T] elementwise when mag is not
 * null), divided by the window sum-of-squares envelope where it exceeds the smallest normal fp32, the n_fft/2
 * centre padding trimmed; 1 <= L <= (T + 1) * hop.  Gather form, fixed order: bitwise repeatable.
 * ldm_griffinlim: n_iter iterations of  y = istft(mag * angles); r = stft(y); angles = unit(r - m/(1+m) r_prev);
 * r_prev = r  from angles = init_angles [B, F, T] complex, then y [B, L] = istft(mag * angles); L must give T
 * frames.  Two launches per iteration on `stream`, no host synchronisation or allocation (capturable); workspace:
 * ldm_griffinlim_workspace(B, n_fft, T) floats.
 * ldm_griffinlim_anchored: the same loop, workspace and launch sequence with the phase pulled towards anchor_phase
 * [B, F, T] complex (unit modulus) by anchor_w [B, F, T] in [0, 1]: every iteration stores
 * unit(a anchor_phase + (1 - a) angles): angles itself where a == 0, anchor_phase itself where a == 1 (bitwise).
 * ldm_mel_project: mel [B, n_mels, T] = M . P [B, F, T]; M [n_mels, F] dense, lohi [n_mels][2] each row's
 * non-zero run [lo, hi).
 * ldm_power_to_db: per item b of x [B, n]: 10 log10(max(x, amin)) - 10 log10(max(amin, max_b x)), clamped below at
 * -top_db when top_db >= 0; workspace: B floats.  ldm_db_to_power: 10^(x / 10).
 * ldm_mel_invert: x [B, F, T] = max(Minv . mel, 0), then `iters` steps  x = max(x - Mt (M x - mel) * inv_lambda, 0),
 * then sqrt when take_sqrt; Mt [F, n_mels] = M transposed, Minv [F, n_mels]; workspace: B * n_mels * T floats. */
int64_t ldm_stft_table_floats(int32_t n_fft);
int ldm_stft_fill_tables(int32_t n_fft, float* host_tables);
int ldm_stft(const float* y, int32_t B, int64_t L, int32_t n_fft, int32_t hop, const float* tables, float* S,
             float* mag, int32_t power, void* stream);
int ldm_istft(const float* S, const float* mag, float* y, int32_t B, int32_t T, int64_t L, int32_t n_fft,
              int32_t hop, const float* tables, void* stream);
int64_t ldm_griffinlim_workspace(int32_t B, int32_t n_fft, int32_t T);
int ldm_griffinlim(const float* mag, const float* init_angles, float* y, int32_t B, int32_t T, int64_t L,
                   int32_t n_fft, int32_t hop, int32_t n_iter, float momentum, const float* tables,
                   float* workspace, void* stream);
int ldm_griffinlim_anchored(const float* mag, const float* init_angles, const float* anchor_phase,
                            const float* anchor_w, float* y, int32_t B, int32_t T, int64_t L, int32_t n_fft,
                            int32_t hop, int32_t n_iter, float momentum, const float* tables, float* workspace,
                            void* stream);
int ldm_mel_project(const float* P, const float* M, const int32_t* lohi, float* mel, int32_t B, int32_t F,
                    int32_t n_mels, int32_t T, void* stream);
int ldm_power_to_db(const float* x, float* out, int32_t B, int64_t n, float amin, float top_db, float* workspace,
                    void* stream);
int ldm_db_to_power(const float* x, float* out, int64_t n, void* stream);
int ldm_mel_invert(const float* mel, const float* M, const float* Mt, const float* Minv, const int32_t* lohi,
                   float inv_lambda, int32_t iters, int32_t take_sqrt, float* x, float* workspace, int32_t B,
                   int32_t F, int32_t n_mels, int32_t T, void* stream);

/* ---- content-anchored vocoder (vocoder.hip) ------------------------------------------------
 * The transfer as an edit of the content's STFT C [B, F, T] complex.  mel_out, mel_content [B, n_mels, T] mel power
 * (the content's after the same round trip as the output's); Wn [n_mels, F] the filterbank divided by its column
 * sums (0 in a column whose sum is 0); mlohi [F][2] each bin's run [m_lo, m_hi) of filters with a non-zero weight
 * (empty: the bin's gain is 1); eps [B] on the device, one positive floor per item.
 *   g = clamp(sum_m Wn[m, f] (mel_out + eps) / (mel_content + eps), 0, max_gain),   Pm = g |C|^2
 *   mag = sqrt(Pm + residual)   (residual [B, F, T] power, or null),   phase0 = C / |C|   ((1, 0) where |C| is below
 *   the smallest normal fp32),   anchor = clamp(1 - |10 log10((mag^2 + eps) / (|C|^2 + eps))| / anchor_db, 0, 1)
 *   (0 everywhere when anchor_db <= 0).
 * ldm_mel_gain_power writes Pm, ldm_mel_gain_target writes mag, phase0 (complex) and anchor; one launch each, one
 * lane per bin, no workspace, no host synchronisation (capturable). */
int ldm_mel_gain_power(const float* C, const float* mel_out, const float* mel_content, const float* Wn,
                       const int32_t* mlohi, const float* eps, float max_gain, float* Pm, int32_t B, int32_t F,
                       int32_t n_mels, int32_t T, void* stream);
int ldm_mel_gain_target(const float* C, const float* mel_out, const float* mel_content, const float* Wn,
                        const int32_t* mlohi, const float* eps, float max_gain, float anchor_db,
                        const float* residual, float* mag, float* phase0, float* anchor, int32_t B, int32_t F,
                        int32_t n_mels, int32_t T, void* stream);

/* ---- harmonic / percussive separation (hpss.hip) -------------------------------------------
 * ldm_median_filter: the running median of x [B, F, T] along time (axis 1) or frequency (axis 0), win odd in 1..63,
 * the axis continued by reflection with the edge sample repeated (d c b a | a b c d | d c b a, period 2n; scipy's
 * mode="reflect"), so an axis shorter than the window reflects several times.  out[i] is the middle order statistic
 * of the window, selected by rank with a position tie-break: always one of the inputs, bitwise
 * scipy.ndimage.median_filter whatever the ties; win = 1 copies.  NaN inputs: unspecified.  out must not overlap x.
 * B <= 65535, F <= 262140, T < 2^30.  One launch, no workspace, no atomics.  ldm_median_tile(axis): the outputs a
 * block covers along the filtered axis (0 for a bad axis).
 * ldm_hpss_masks: librosa's soft masks of n elements, every step a rounded fp32 operation (no contraction):
 *   mask_h = soft(harm, margin_h perc),  mask_p = soft(perc, margin_p harm),
 *   soft(X, R) = (X/Z)^p / ((X/Z)^p + (R/Z)^p),  Z = max(X, R);  0.5 where Z is below the smallest normal fp32.
 * p = 1 and p = 2 multiply, any other finite p > 0 calls powf; margins >= 1; either output may be null.
 * ldm_mask_mel_share: a bin-domain mask [B, F, T] carried to the mel grid as the energy share of what it selects,
 *   out[b, m, t] = (sum_f M[m, f] mask[b, f, t] P[b, f, t]) / (sum_f M[m, f] P[b, f, t]),  f in [lo_m, hi_m),
 * P [B, F, T] power, M [n_mels, F] and lohi [n_mels][2] as ldm_mel_project's; 0.5 where the denominator is below the
 * smallest normal fp32.  Both sums add the same products in the same ascending order, so a mask in [0, 1] gives a
 * share in [0, 1] (clamped to it), mask == 1 gives 1 and mask == 0 gives 0 exactly.  One launch. */
int ldm_median_tile(int32_t axis);
int ldm_median_filter(const float* x, int32_t B, int32_t F, int32_t T, int32_t axis, int32_t win, float* out,
                      void* stream);
int ldm_hpss_masks(const float* harm, const float* perc, int64_t n, float power, float margin_h, float margin_p,
                   float* mask_h, float* mask_p, void* stream);
int ldm_mask_mel_share(const float* P, const float* mask, const float* M, const int32_t* lohi, int32_t B, int32_t F,
                       int32_t T, int32_t n_mels, float* out, void* stream);

/* ---- transfer report: feature kernels of the scores (metrics.hip) ---------------------------
 * Spectra are [B, rows, T] with T contiguous.  The fp32 entries do every step as one rounded fp32 operation in the
 * stated order (no contraction); the float64 entries have a fixed partition that depends on the item's own length
 * only and a fixed order, so they are bitwise repeatable and item b's result does not depend on the other items.
 * ldm_onset_strength: db [B, n_mels, T] (a log-mel in dB), lag >= 1 -> env [B, T],
 *   env[b, t] = (sum_m max(0, db[b, m, t] - db[b, m, t - lag])) / n_mels for t >= lag (m ascending), 0 for t < lag;
 *   T <= lag gives all zeros.  One launch.
 * ldm_chroma: P [B, F, T] power; bin f adds wt[f] P to pitch class cls[f] and (1 - wt[f]) P to class (cls[f] + 1) % 12,
 *   bins ascending; cls[f] < 0: the bin contributes nothing.  chroma [B, 12, T]: each frame divided by its L2 norm
 *   over the classes, exactly 0 where the norm is below the smallest normal fp32.  P is read once.  One launch.
 * ldm_mfcc_moments: db [B, n_mels, T] fp32, D [n_mfcc, n_mels] float64 on the device (n_mfcc <= 32), w [B, T] fp32
 *   frame weights or NULL (all 1) -> mom [B][1 + n_mfcc + n_mfcc (n_mfcc + 1) / 2] float64:
 *   { sum_t w, sum_t w c_k (k ascending), sum_t w c_j c_k (j <= k, row-major) }, c_k(t) = sum_m D[k, m] db[m, t].
 *   Float64 throughout; the coefficients are never written to memory.  workspace: ldm_mfcc_moments_workspace(B, T,
 *   n_mfcc) doubles (0 for bad arguments).  Two launches.
 * ldm_pair_stats: a, b [B, n] fp32, w [B, n] fp32 or NULL (all 1) -> out [B][7] float64:
 *   { sum w, sum w a, sum w b, sum w a^2, sum w b^2, sum w a b, sum w (a - b)^2 }, operands converted to float64
 *   first.  workspace: ldm_pair_stats_workspace(B, n) doubles.  Two launches. */
int ldm_onset_strength(const float* db, int32_t B, int32_t n_mels, int32_t T, int32_t lag, float* env, void* stream);
int ldm_chroma(const float* P, const int32_t* cls, const float* wt, int32_t B, int32_t F, int32_t T, float* chroma,
               void* stream);
int64_t ldm_mfcc_moments_workspace(int32_t B, int32_t T, int32_t n_mfcc);
int ldm_mfcc_moments(const float* db, const double* D, const float* w, int32_t B, int32_t n_mels, int32_t T,
                     int32_t n_mfcc, double* mom, double* workspace, void* stream);
int64_t ldm_pair_stats_workspace(int32_t B, int64_t n);
int ldm_pair_stats(const float* a, const float* b, const float* w, int32_t B, int64_t n, double* out, double* workspace,
                   void* stream);

/* ---- loudness: BS.1770 meter, true peak, look-ahead limiter (loudness.hip) -------------------
 * Mono fp32 recordings x [B, L]; rows are independent.  No entry synchronises or allocates.
 * ldm_loudness_hop_sums: hop_sums [B, L / hop] float64 = the sum of squares of the K-weighted signal over consecutive
 *   hops of `hop` samples (round(0.1 sr)).  sos: 10 HOST doubles {b0, b1, b2, a1, a2} of the shelf, then of the
 *   high-pass (a0 = 1; ldm_amd.audio.k_weighting).  Float64 throughout; the recursion is cut into chunks of
 *   ldm_loudness_chunk(hop) samples whose true start states one small launch carries across (three launches); every
 *   hop sum is added in sample order: bitwise repeatable and independent of B.  workspace:
 *   ldm_loudness_workspace(B, L, hop) doubles.  L < hop writes nothing.
 * ldm_loudness_gate: out [B, 4] float64 = {integrated LUFS, blocks passing both gates, relative threshold, blocks in
 *   all} from hop_sums [B, n_hops]: blocks of 4 hops (400 ms, 75 % overlap), l_j = -0.691 + 10 log10(z_j) with z_j the
 *   block's mean square, the absolute gate l_j > -70, the relative gate 10 LU under the loudness of the absolutely-gated
 *   mean.  No block passing (n_hops < 4, silence): -inf, and a relative threshold of -inf when none passes the absolute
 *   gate.  One block per row.
 * ldm_loudness_gain: y = x 10^((target_lufs - stats[b][0]) / 20) with stats ldm_loudness_gate's out; a row whose
 *   loudness is not finite gets 0 dB (y bitwise x).  gain_db [B] float64 receives the decibels applied.
 * ldm_true_peak: out [B] = max(max |x[n]|, max |4x oversampled x|), the oversampling being ldm_resample_f32's with
 *   taps [4, 2W+1] (up must be 4, W <= 256), fused with the maximum: the 4x signal is never written.  Bitwise
 *   repeatable.  workspace: ldm_true_peak_workspace(B, L) floats.
 * ldm_limit: the look-ahead true-peak limiter, one fused launch.  With c = ceiling in (0, 1] and Lh = lookahead:
 *   p[n] = max(|x[n]|, |the four oversampling phases at n|), x = 0 outside [0, L);  r[n] = min(1, c / p[n]), 1 outside
 *   [0, L);  m[n] = min_{|j| <= Lh} r[n + j] on [-Lh, L - 1 + Lh];  g[n] = 1 - sum_{|j| <= Lh} w_j (1 - m[n + j]), w the
 *   2 Lh + 1 non-zero points of a Hann window normalised to sum 1;  y[n] = g[n] x[n].  g <= r in exact arithmetic; where
 *   nothing exceeds c, g is exactly 1 and y bitwise x.  A block holds ldm_limit_tile() samples and a halo of 2 Lh + W
 *   in LDS, so lookahead <= LDM_LIMIT_MAX_LOOKAHEAD at W = 34 (3 tile + 12 Lh + 10 W + 37 floats within 160 KiB; more is
 *   an error).  gain [B, L] (or NULL) receives g; min_gain [B] (or NULL) its minimum per row, which needs workspace:
 *   ldm_limit_workspace(B, L) floats.  y and gain must not alias x.
 * ldm_peak_trim: in place, y[b] *= s_b with s_b = 1 where true_peak[b] <= ceiling and (ceiling / true_peak[b])
 *   (1 - 2^-15) otherwise (the margin covers the rounding of a second fp32 true-peak evaluation, 2 x 70 x 2.31 x 2^-24);
 *   trim [B] (or NULL) receives s_b. */
#define LDM_LIMIT_MAX_LOOKAHEAD 1333
int32_t ldm_loudness_chunk(int32_t hop);
int64_t ldm_loudness_workspace(int32_t B, int64_t L, int32_t hop);
int ldm_loudness_hop_sums(const float* x, int32_t B, int64_t L, int32_t hop, const double* sos, double* hop_sums,
                          double* workspace, void* stream);
int ldm_loudness_gate(const double* hop_sums, int32_t B, int32_t n_hops, int32_t hop, double* out, void* stream);
int ldm_loudness_gain(const float* x, const double* stats, double target_lufs, int32_t B, int64_t L, float* y,
                      double* gain_db, void* stream);
int64_t ldm_true_peak_workspace(int32_t B, int64_t L);
int ldm_true_peak(const float* x, int32_t B, int64_t L, const float* taps, int32_t up, int32_t W, float* out,
                  float* workspace, void* stream);
int32_t ldm_limit_tile(void);
int64_t ldm_limit_workspace(int32_t B, int64_t L);
int ldm_limit(const float* x, int32_t B, int64_t L, const float* taps, int32_t up, int32_t W, int32_t lookahead,
              float ceiling, float* y, float* gain, float* min_gain, float* workspace, void* stream);
int ldm_peak_trim(float* y, const float* true_peak, float ceiling, int32_t B, int64_t L, float* trim, void* stream);

/* ---- resampling and silence trim (resample.hip) -------------------------------------------
 * The rational polyphase resampler  y[n] = sum_{j=-W..W} x[i0 + j] * taps[p][j + W],  i0 = floor(n down / up),
 * p = (n down) mod up, x zero outside [0, L); taps [up, 2W+1] fp32 on the device is the caller's filter (the
 * project's Kaiser-windowed sinc: ldm_amd.audio.resample_taps).  up / down is the reduced ratio sr_out / sr_in.
 * The output has ldm_resample_out_len(L, up, down) = ceil(L up / down) samples per row (0 for bad arguments).
 * One launch, no atomics, every output summed in ascending j: bitwise repeatable and independent of B.
 * ldm_resample_f32: x [B, L] -> y [B, n_out].  ldm_resample_pcm16: interleaved int16 pcm [L, channels] -> y [n_out],
 * each frame decoded as the mean over channels of s / 32768 in the load (bitwise the float form of that signal for
 * 1 and 2 channels).  Ratios whose tile does not fit (up > 1024, or about 4 down + 2 W > 8192) are refused.
 * ldm_trim_bounds: librosa.effects.trim's bounds per row of y [B, L]: frames t < 1 + L / hop cover
 * [t hop - frame_length/2, t hop + frame_length/2) with zero padding, ms[t] their mean square; a frame is
 * non-silent when max(ms[t], 1e-10) > max(max_t ms, 1e-10) * 10^(-top_db / 10); bounds[b] = {hop * first,
 * min(L, hop * (last + 1))} as int64 on the device, {0, 0} when no frame passes or max_t ms <= 1e-10.
 * workspace: ldm_trim_workspace_floats(B, L, hop) floats.  Two launches, no host synchronisation. */
int64_t ldm_resample_out_len(int64_t L, int32_t up, int32_t down);
int ldm_resample_f32(const float* x, int32_t B, int64_t L, const float* taps, int32_t up, int32_t down, int32_t W,
                     float* y, void* stream);
int ldm_resample_pcm16(const int16_t* pcm, int64_t L, int32_t channels, const float* taps, int32_t up, int32_t down,
                       int32_t W, float* y, void* stream);
int64_t ldm_trim_workspace_floats(int32_t B, int64_t L, int32_t hop);
int ldm_trim_bounds(const float* y, int32_t B, int64_t L, int32_t frame_length, int32_t hop, float top_db,
                    float* workspace, int64_t* bounds, void* stream);

/* ---- whole-recording windows (longform.hip) ------------------------------------------------
 * The window plan of a recording of T_total mel frames: N = max(1, ceil((T_total - overlap) / stride)) windows of
 * `frames` frames, stride = frames - overlap; window n covers frames [n stride, n stride + frames), frames at or
 * beyond T_total hold zero power.  frames is a multiple of 64 and 0 <= overlap <= frames / 2 (at most two windows
 * cover a frame).  ldm_mel_window_count returns N, 0 for a bad plan.
 * ldm_mel_windows: P [n_mels, T_total] mel power -> x [N, 1, n_mels, frames], the model's [0,1] input of each
 * window, and ref_db [N] = 10 log10(max(amin, max of window n)); x is bitwise ldm_u8_to_unit(ldm_mel_quantize(
 * ldm_power_to_db(window n, amin, top_db), max_db)) of the zero-padded window.  Two launches, no unfolded copy.
 * ldm_mel_stitch: y [N, 1, n_mels, frames] decoded windows -> power [n_mels, T_total] = 10^(db / 10) and, when db
 * is not null, db [n_mels, T_total]; with d(n, j) = clamp(y[n, 0, m, j], 0, 1) max_db - max_db + ref_db[n],
 * n1 = min(N - 1, t / stride), j1 = t - n1 stride:  db = d(n1, j1), or inside an overlap (n1 >= 1, j1 < overlap)
 * ((overlap - j1) d(n1 - 1, j1 + stride) + (j1 + 1) d(n1, j1)) / (overlap + 1).  N must be the plan's count.
 * One launch, gather form, no atomics: bitwise repeatable. */
int64_t ldm_mel_window_count(int64_t T_total, int32_t frames, int32_t overlap);
int ldm_mel_windows(const float* P, int32_t n_mels, int64_t T_total, int32_t frames, int32_t overlap, float amin,
                    float top_db, float max_db, float* x, float* ref_db, void* stream);
int ldm_mel_stitch(const float* y, const float* ref_db, int32_t N, int32_t n_mels, int32_t frames, int32_t overlap,
                   int64_t T_total, float max_db, float* power, float* db, void* stream);

/* ---- step kernels (uconv.hip): fixed-structure implicit GEMMs of the nine UNet convs -------------------
 * Packed size (floats) of layer `layer` (0..8 = enc1..dec1) and its packing from the torch weight layout
 * (conv [Cout][Cin][3][3], transposed conv [Cin][Cout][3][3]).  ldm_step_conv runs one layer on NHWC
 * activations (latent [B,H,W] with H, W multiples of 8): y = act(conv(x) + bias) (+ bcast[b][c] for
 * enc2) (+ skip for dec4..dec2); bias is [Cout], or [Hout*Wout][Cout] for the folded enc4 / bottleneck.
 * dec1 only runs fused with the sampler's update inside ldm_sample. */
int64_t ldm_step_packed_floats(int32_t layer);
int ldm_step_pack_weight(int32_t layer, const float* w, float* packed, void* stream);
/* The pack for an operand precision: LDM_DT_F32 as ldm_step_pack_weight; LDM_DT_F16 / LDM_DT_BF16 write the
 * same layout in 16-bit elements (ldm_step_packed_floats / 2 floats of storage), which is what every step
 * conv with that dtype reads (ldm_step_conv_dt, _ws, ldm_step_dec1_ddim, ldm_unet_weights.step_w). */
int ldm_step_pack_weight_dt(int32_t layer, int32_t dtype, const float* w, float* packed, void* stream);
int ldm_step_conv(int32_t layer, int32_t B, int32_t H, int32_t W, const float* x, const float* packed,
                  const float* bias, const float* bcast, const float* skip, float* y, void* stream);
/* The step kernels of the deep layers (enc3, enc4, bottleneck, dec4, dec3) also come in a K-split form: a
 * 32x32 block tile with K split over 2-8 blocks (write-through partial tiles, the last block of a tile sums
 * them in split order), half the operand bytes per block.  It runs when a workspace is given (and
 * LDM_UCONV_KS, a layer bit mask, selects the layer; default all five): ldm_step_workspace_floats(B, H, W)
 * floats, zero-filled once (its counters return to zero after every launch); launches on one stream may
 * share it.  ldm_step_conv / ldm_step_conv_dt run the single-block form. */
int64_t ldm_step_workspace_floats(int32_t B, int32_t H, int32_t W);
/* The leading part of that workspace that holds the split-K tile counters (one int32 per tile of the layer with
 * the most tiles, rounded up to 64): zero between launches, like the 64 layer-pair counters at its end. */
int64_t ldm_step_workspace_counter_floats(int32_t B, int32_t H, int32_t W);
int ldm_step_conv_ws(int32_t layer, int32_t B, int32_t H, int32_t W, const float* x, const float* packed,
                     const float* bias, const float* bcast, const float* skip, float* y, int32_t dtype,
                     float* workspace, void* stream);
/* dec1 with the fused DDIM update, as the reverse loop runs it: d2 [B,H,W,64] NHWC, xs [B,H,W,32] NHWC sampler
 * state updated in place, coef [4] {sqrt(ab_t), sqrt(1-ab_t), sqrt(ab_next), sqrt(1-ab_next)}, x0_log /
 * eps_log NCHW [B,32,H,W] or NULL (model.py:442-463). */
int ldm_step_dec1_ddim(int32_t B, int32_t H, int32_t W, const float* d2, const float* packed, const float* bias,
                       const float* coef, float eta, float* xs, float* x0_log, float* eps_log, int32_t dtype,
                       void* stream);
/* Its twin with the multistep update (ldm_msolver_step's arithmetic, fp32 whatever dtype is): coef [8]; x0_prev
 * (NCHW like the logs, or NULL) is read with the stride x0_log is written with; x0_log is required. */
int ldm_step_dec1_msolver(int32_t B, int32_t H, int32_t W, const float* d2, const float* packed, const float* bias,
                          const float* coef, float* xs, const float* x0_prev, float* x0_log, float* eps_log,
                          int32_t dtype, void* stream);
/* Which reverse-loop layers run uconv.hip's K-split form (bit l = layer l; LDM_UCONV_KS, default enc4 +
 * bottleneck + dec4); every other layer runs the single-block form. */
int ldm_step_layer_forms(int32_t* ks_layers);
/* ldm_step_conv with an operand precision LDM_DT_* (ldm_step_conv = LDM_DT_F32). */
int ldm_step_conv_dt(int32_t layer, int32_t B, int32_t H, int32_t W, const float* x, const float* packed,
                     const float* bias, const float* bcast, const float* skip, float* y, int32_t dtype, void* stream);

/* ---- train step backward (LDMTrainer.train_step, train.py:163-208: scaler.scale(loss).backward()) ---
 * Data gradients of a conv are the forward kernel on the dual descriptor (conv <-> transposed conv);
 * these are the remaining pieces.  All reductions are fixed-order (bitwise reproducible). */
/* dW of nn.Conv2d / nn.ConvTranspose2d for descriptor d (the FORWARD descriptor): x = layer input,
 * dy = gradient at the layer's pre-epilogue output.  dw in the torch weight layout; accumulate != 0 adds.
 * workspace: ldm_conv_wgrad_workspace_floats(d) floats. */
int64_t ldm_conv_wgrad_workspace_floats(const ldm_conv_desc* d);
/* ldm_conv_backward_weight with an operand precision LDM_DT_* (the tap-shared kernel rounds x and dy;
 * shapes it does not cover run the fp32 kernel). */
int ldm_conv_backward_weight_dt(const ldm_conv_desc* d, const float* x, const float* dy, float* dw,
                                int32_t accumulate, float* workspace, int32_t dtype, void* stream);
/* ldm_conv_backward_weight_dt with a tap-shared gradient's split-K reduction deferred (the train step's weight
 * gradients are read only by the optimizer): the partials stay in `workspace` (ldm_conv_wgrad_workspace_floats,
 * kept until the reduction) and *splits_out receives their count S (0: nothing deferred, dw written).
 * ldm_wgrad_reduce_many then reduces every job in one launch per 24 jobs, bitwise ldm_conv_backward_weight_dt's
 * result (MN = the gradient's element count, a multiple of 4; partial and dw 16-byte aligned). */
int ldm_conv_backward_weight_defer(const ldm_conv_desc* d, const float* x, const float* dy, float* dw,
                                   int32_t accumulate, float* workspace, int32_t dtype, int32_t* splits_out,
                                   void* stream);
typedef struct ldm_wgrad_red_job {
    const float* partial;   /* [S][MN] */
    float* dw;              /* [MN] */
    int32_t S, MN, accumulate;
} ldm_wgrad_red_job;
int ldm_wgrad_reduce_many(const ldm_wgrad_red_job* jobs, int32_t n, void* stream);
/* The 16-bit storage flags (LDM_DT_X16 | LDM_DT_DY16) ldm_conv_backward_weight_dt takes for d at a 16-bit
 * operand precision (0: neither; the caller then passes fp32 tensors). */
int32_t ldm_conv_wgrad_storage16(const ldm_conv_desc* d);
int ldm_conv_backward_weight(const ldm_conv_desc* d, const float* x, const float* dy, float* dw, int32_t accumulate,
                             float* workspace, void* stream);
/* Backward of the fused epilogue act(v) (+bcast[b,c]) (+skip): dv = dy*act'(v) (from act_out = act(v);
 * GELU from pre_act = v), dbias[c] = sum dv, dbcast[b,c] = sum_hw dy.  dv / dbias / dbcast may be NULL;
 * dv may alias dy.  workspace: ldm_reduce_workspace_floats(B,C,HW) floats (NULL when no sums). */
int ldm_act_backward(const float* dy, const float* act_out, const float* pre_act, int32_t act, int32_t B, int32_t C,
                     int32_t HW, float* dv, float* dbias, float* dbcast, float* workspace, void* stream);
/* ldm_act_backward with the bias gradient's finalize deferred (the train step's convs: their bias gradients are read
 * only by the optimizer): the slice partials go to `workspace` (ldm_act_partial_floats(B, C, HW) floats, kept until
 * the finalize), *q_out receives their slice count for the job (0: nothing deferred — the small-plane kernel
 * wrote dbias itself).  No bcast gradient.  ldm_act_finalize_many then writes every job's dbias in one launch per 24
 * jobs, bitwise what ldm_act_backward writes. */
int ldm_act_backward_defer(const float* dy, const float* act_out, const float* pre_act, int32_t act_code, int32_t B,
                           int32_t C, int32_t HW, float* dv, float* dbias, float* workspace, int32_t* q_out, void* stream);
int64_t ldm_act_partial_floats(int32_t B, int32_t C, int32_t HW);
typedef struct ldm_act_fin_job {
    const float* part;   /* the deferred call's partials */
    float* dbias;        /* [C]: the sums */
    int32_t B, C, Q;     /* Q: the call's *q_out (kind 1: *p_out) */
    int32_t kind;        /* 0: ldm_act_backward_defer; 1: ldm_batchnorm_backward_dxsum_defer's dx sum */
} ldm_act_fin_job;
int ldm_act_finalize_many(const ldm_act_fin_job* jobs, int32_t n, void* stream);
/* train-mode BatchNorm2d (+ReLU/Tanh) backward from the saved batch stats of ldm_batchnorm_train:
 * y = its output, x = its input, weight / bias its affine parameters (NULL = 1 / 0); dx / dweight / dbias
 * may be NULL.  y may be NULL when act is NONE or RELU: the ReLU mask is then re-evaluated from x with the
 * forward's own arithmetic (one tensor read less per pass).  workspace as ldm_batchnorm_train. */
int ldm_batchnorm_backward(const float* dy, const float* y, const float* x, const float* save_mean,
                           const float* save_invstd, const float* weight, const float* bias, int32_t act, int32_t B,
                           int32_t C, int32_t HW, float* dx, float* dweight, float* dbias, float* workspace,
                           void* stream);
/* ldm_batchnorm_backward (dx required) that also writes dx_sum[c] = the sum of dx (as stored) over (b, h, w): the
 * bias gradient of the conv whose output x is, without a sweep of its own over dx (round 6).  workspace as
 * ldm_batchnorm_train (ldm_reduce_workspace_floats covers the extra slice partials). */
int ldm_batchnorm_backward_dxsum(const float* dy, const float* y, const float* x, const float* save_mean,
                                 const float* save_invstd, const float* weight, const float* bias, int32_t act,
                                 int32_t B, int32_t C, int32_t HW, float* dx, float* dweight, float* dbias,
                                 float* dx_sum, float* workspace, void* stream);
/* ldm_batchnorm_backward_dxsum with the dx sum's finalize deferred to ldm_act_finalize_many (a job of kind 1 with
 * part = dxs_part, dbias = dx_sum, Q = *p_out); dxs_part holds ldm_bn_dxsum_partial_floats(B, C, HW) floats. */
int ldm_batchnorm_backward_dxsum_defer(const float* dy, const float* y, const float* x, const float* save_mean,
                                       const float* save_invstd, const float* weight, const float* bias, int32_t act_code,
                                       int32_t B, int32_t C, int32_t HW, float* dx, float* dweight, float* dbias,
                                       float* dx_sum, float* dxs_part, int32_t* p_out, float* workspace, void* stream);
int64_t ldm_bn_dxsum_partial_floats(int32_t B, int32_t C, int32_t HW);
/* The same in two stages for SyncBatchNorm: sums[2c] = sum g, sums[2c+1] = sum g*xhat over this rank
 * (g = dy*act'(y)) and sums[2C] = this rank's B*H*W (sums holds 2C+1 doubles); dbias / dweight get the
 * local sums (parameter grads stay local, as in torch.nn.SyncBatchNorm; the DP gradient all-reduce
 * averages them) -> the caller all-reduces all 2C+1 doubles -> apply (count <= 0: read sums[2C]). */
int ldm_batchnorm_backward_reduce(const float* dy, const float* y, const float* x, const float* save_mean,
                                  const float* save_invstd, const float* weight, const float* bias, int32_t act,
                                  int32_t B, int32_t C, int32_t HW, double* sums, float* dweight, float* dbias,
                                  float* workspace, void* stream);
int ldm_batchnorm_backward_apply(const float* dy, const float* y, const float* x, const float* save_mean,
                                 const float* save_invstd, const float* weight, const float* bias, int32_t act,
                                 int32_t B, int32_t C, int32_t HW, const double* sums, double count, float* dx,
                                 void* stream);
/* Backward of ldm_attention_core: dq [B,E,L], dkv [B,2E,S] (dK then dV). */
int ldm_attention_backward(const float* q, const float* kv, const float* dout, float* dq, float* dkv, int32_t B,
                           int32_t E, int32_t heads, int32_t L, int32_t S, float scale, void* stream);
/* 1 when ldm_attention_backward has a form for the shape (the MFMA form: L, S and the head dim multiples of 16
 * within 160 KiB of LDS; the scalar form: (d*L + d*S + 2*L*S) floats within 64 KiB), 0 when it would fail with
 * "head tile exceeds LDS budget" (e.g. d = 128 at L = S = 50); those shapes go to the pair
 * ldm_attention_forward_lse / ldm_attention_backward_flash where the head dim allows. */
int ldm_attention_backward_supported(int32_t E, int32_t heads, int32_t L, int32_t S);
/* The same backward for any L, S (flash.hip), from the forward's out and lse (ldm_attention_forward_lse):
 * delta = rowsum(dO * O) into delta_ws [B,heads,L], then dK/dV (64 keys per block, q and dO streamed) and
 * dQ (64 queries per block, K and V streamed), deterministic. */
int ldm_attention_backward_flash(const float* q, const float* kv, const float* out, const float* lse,
                                 const float* dout, float* dq, float* dkv, float* delta_ws, int32_t B, int32_t E,
                                 int32_t heads, int32_t L, int32_t S, float scale, void* stream);

/* ---- multi-tensor weight re-pack (the train step refreshes every packed trainable conv weight after the
 * optimizer step in one launch instead of one per weight; pack.hip).  ldm_pack_many_prepare fills
 * n * ldm_pack_job_bytes() bytes of host_jobs with the jobs for (descs[i], plans[i]) reading the torch-layout
 * weight w[i] into out[i] (the buffer ldm_conv_pack_weight would fill, kinds 1-3) and returns the launch
 * size; copy the table to device memory once, then ldm_pack_many(table, n, launch_size, stream) re-packs
 * them all (same values as ldm_conv_pack_weight). */
int64_t ldm_pack_job_bytes(void);
int ldm_pack_many_prepare(const ldm_conv_desc* descs, const ldm_conv_plan* plans, const float* const* w,
                          void* const* out, int32_t n, void* host_jobs, int64_t* launch_size);
int ldm_pack_many(const void* device_jobs, int32_t n, int64_t launch_size, void* stream);

/* ---- LPIPS-AlexNet perceptual distance (loss.py:6-21: lpips==0.1.4 LPIPS(net='alex') on 2x-1)
 * The AlexNet convs run on ldm_conv_forward: 3x3 directly, 11x11/s4 and 5x5 as ldm_im2col + a 1x1 conv (their
 * data gradient: the 1x1 dual conv + ldm_col2im).  col [B,Kpad,Ho,Wo], k = (c*kh+ky)*kw+kx, rows >= Cv*kh*kw
 * zero.  shift/scale (or NULL): the LPIPS ScalingLayer fused, a 1-channel input broadcast to Cv channels
 * (t - shift_c)/scale_c; unit=1 first maps x -> 2x - 1 (perceptual_loss_old); col2im folds both back into dx.
 * ldm_maxpool3s2: nn.MaxPool2d(3, 2) (floor); its backward routes dy to torch's first-occurrence argmax.
 * ldm_lpips_layer: val[b] += mean_p sum_c w_c (f0_c/(|f0|+1e-10) - f1_c/(|f1|+1e-10))^2 (normalize_tensor,
 * squared difference, 1x1 lin head without bias, spatial average); workspace >= B*HW floats.
 * ldm_lpips_layer_backward: d val / d f1 (side 1) or d f0 (side 0) times gval[b], written or accumulated. */
int ldm_im2col(const float* x, int32_t B, int32_t C, int32_t H, int32_t W, int32_t kh, int32_t kw, int32_t stride,
               int32_t pad, int32_t Kpad, const float* shift, const float* scale, int32_t Cv, int32_t unit, float* col,
               void* stream);
int ldm_col2im(const float* col, int32_t B, int32_t C, int32_t H, int32_t W, int32_t kh, int32_t kw, int32_t stride,
               int32_t pad, int32_t Kpad, const float* scale, int32_t Cv, int32_t unit, float* dx, void* stream);
int ldm_maxpool3s2(const float* x, float* y, int32_t B, int32_t C, int32_t H, int32_t W, void* stream);
int ldm_maxpool3s2_backward(const float* x, const float* dy, float* dx, int32_t B, int32_t C, int32_t H, int32_t W,
                            void* stream);
int ldm_lpips_layer(const float* f0, const float* f1, const float* w, int32_t B, int32_t C, int32_t HW, float* val,
                    float* workspace, void* stream);
int ldm_lpips_layer_backward(const float* f0, const float* f1, const float* w, const float* gval, int32_t B,
                             int32_t C, int32_t HW, int32_t side, int32_t accumulate, float* df, void* stream);

/* ---- VGGish feature / style loss (loss.py:52-101, VGGishFeatureLoss.forward) ----
 * The conv stack runs on ldm_conv_forward (ReLU fused: each conv launch yields one feature tap).
 * ldm_maxpool2x2: nn.MaxPool2d(2, 2) on NCHW fp32 (floor mode, NaN-propagating), y [B,C,H/2,W/2].
 * ldm_std_mse_moments: per sample b of p, t [B][n] (n = C*H*W contiguous): moments[b][0..4] = sum p,
 *   sum p^2, sum t, sum t^2, sum p*t (fp64, fixed slices and order; workspace
 *   ldm_std_mse_workspace_floats(B, n) floats, 8-byte aligned).
 * ldm_std_mse_accumulate: *acc += scale * mse(p / (std(p) + eps), t / (std(t) + eps)) from the moments
 *   (torch.std per sample over dims 1..3, unbiased), and *out = (float)*acc when out is not NULL. */
int ldm_maxpool2x2(const float* x, float* y, int32_t B, int32_t C, int32_t H, int32_t W, void* stream);
int64_t ldm_std_mse_workspace_floats(int32_t B, int64_t n);
int ldm_std_mse_moments(const float* p, const float* t, int32_t B, int64_t n, double* moments, float* workspace,
                        void* stream);
int ldm_std_mse_accumulate(const double* moments, int32_t B, int64_t n, double eps, double scale, double* acc,
                           float* out, void* stream);

/* ---- optimiser: torch.optim.Adam (train.py:156) + torch.amp.GradScaler (train.py:157,189-201) ----
 * Multi-tensor: `slots` (device array) lists the parameters; the work is cut into chunks of
 * chunk_len elements, chunk i covering slots[chunk_tensor[i]] from element chunk_start[i]. */
typedef struct ldm_tensor_slot {
    float* param;
    float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t numel;
} ldm_tensor_slot;
/* scaler.unscale_: grad *= inv_scale[0] (device scalar, NULL = 1); found_inf[0] |= any non-finite. */
int ldm_unscale_check(const ldm_tensor_slot* slots, const int32_t* chunk_tensor, const int64_t* chunk_start,
                      int32_t nchunks, int32_t chunk_len, const float* inv_scale, int32_t* found_inf, void* stream);
/* optimizer.step() (skipped entirely when found_inf[0] != 0, as scaler.step does). step = 1-based.
 * decoupled = 0: torch.optim.Adam (L2 added to the gradient); 1: torch.optim.AdamW (train.py:44).
 * Hyper-parameters are the optimizer's python floats (double); derived scalars are formed in double
 * and cast once to fp32, as torch's Adam does. */
int ldm_adam_step(const ldm_tensor_slot* slots, const int32_t* chunk_tensor, const int64_t* chunk_start,
                  int32_t nchunks, int32_t chunk_len, double lr, double beta1, double beta2, double eps,
                  double weight_decay, int32_t decoupled, int32_t step, const int32_t* found_inf, void* stream);
/* The capturable form of ldm_adam_step (hipGraph-captured train steps, LDMTrainer.graph_step): the step
 * count is the device float step[0], advanced by one only when found_inf[0] == 0 (or found_inf NULL);
 * the derived scalars are formed from it on the device exactly as ldm_adam_step forms them on the host,
 * into the caller's 8-float device workspace `scalars`.  Replaces torch.optim.Adam(capturable=True)'s
 * _single_tensor_adam capturable branch (train.py:156's optimizer when the step is graph-captured). */
int ldm_adam_step_dev(const ldm_tensor_slot* slots, const int32_t* chunk_tensor, const int64_t* chunk_start,
                      int32_t nchunks, int32_t chunk_len, double lr, double beta1, double beta2, double eps,
                      double weight_decay, int32_t decoupled, float* step, const int32_t* found_inf, float* scalars,
                      void* stream);
/* ---- gradient-norm clipping and EMA weights inside the optimizer's launches ----
 * ldm_unscale_check_norm: ldm_unscale_check (same unscale, same flag, inv_scale NULL = 1) that also writes
 *   partials[i] = the sum over chunk i of (double)g * (double)g of its unscaled gradients (device double
 *   [nchunks], 8-byte aligned; fixed-order block reduction, one plain store per chunk, no atomics: two runs give
 *   bitwise equal partials).
 * ldm_grad_norm_finalize: one block; sum = the partials in ascending chunk order in fp64 (associated by runs of
 *   ceil(nchunks / 256) consecutive chunks; nchunks <= 256: strictly one after the other);
 *   out[0] = (float)sqrt(sum); out[1] = (float)min(1, max_norm / (sqrt(sum) + 1e-6)), formed in double:
 *   torch.nn.utils.clip_grad_norm_'s coefficient (NaN for a NaN norm, 0 for +inf).  max_norm <= 0: norm only,
 *   out[1] = 1.  Several param groups: one call over the concatenation of their partials (one global norm). */
int ldm_unscale_check_norm(const ldm_tensor_slot* slots, const int32_t* chunk_tensor, const int64_t* chunk_start,
                           int32_t nchunks, int32_t chunk_len, const float* inv_scale, int32_t* found_inf,
                           double* partials, void* stream);
int ldm_grad_norm_finalize(const double* partials, int64_t nchunks, double max_norm, float* out, void* stream);
/* ldm_adam_step / ldm_adam_step_dev with the options of one record (NULL record, or all fields NULL: exactly
 * the plain entry's launch).  The multiplier is applied to the loaded gradient (.grad in memory is not
 * rewritten); the EMA is updated from the parameter value the step just formed, and is skipped with the step
 * on found_inf. */
typedef struct ldm_adam_ext {
    const float*  grad_mul;  /* device scalar or NULL: g <- g * grad_mul[0], one fp32 multiply, before the weight-decay line */
    float* const* ema;       /* device array, one pointer per slot (same order as slots), or NULL */
    double        ema_decay; /* e <- e + (float)(1 - decay) * (p_new - e) (one fused multiply-add), 0 <= decay < 1 */
} ldm_adam_ext;
int ldm_adam_step_ext(const ldm_tensor_slot* slots, const int32_t* chunk_tensor, const int64_t* chunk_start,
                      int32_t nchunks, int32_t chunk_len, double lr, double beta1, double beta2, double eps,
                      double weight_decay, int32_t decoupled, int32_t step, const int32_t* found_inf,
                      const ldm_adam_ext* ext, void* stream);
int ldm_adam_step_dev_ext(const ldm_tensor_slot* slots, const int32_t* chunk_tensor, const int64_t* chunk_start,
                          int32_t nchunks, int32_t chunk_len, double lr, double beta1, double beta2, double eps,
                          double weight_decay, int32_t decoupled, float* step, const int32_t* found_inf,
                          float* scalars, const ldm_adam_ext* ext, void* stream);
/* The EMA update alone (for callers that step with another optimizer): slot.param = the EMA tensor,
 * slot.grad = the tensor it follows; e <- e + (float)(1 - decay) * (src - e); skipped when found_inf[0] != 0. */
int ldm_ema_update(const ldm_tensor_slot* slots, const int32_t* chunk_tensor, const int64_t* chunk_start,
                   int32_t nchunks, int32_t chunk_len, double decay, const int32_t* found_inf, void* stream);
/* scaler.update(): scale *= backoff on inf (tracker = 0), *= growth after growth_interval clean steps. */
int ldm_update_scale(float* scale, int32_t* growth_tracker, const int32_t* found_inf, float growth_factor,
                     float backoff_factor, int32_t growth_interval, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LDM_CAPI_H */
