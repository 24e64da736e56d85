// Whole-UNet forward (UNet.forward, model.py:196-231) and the DDIM reverse loop
// (style_conditioned_ddim_sample model.py:409-465 / content_style_ddim_sample :503-559) as one C call:
// ~16 launches per denoising step, no host synchronisation, no allocation — the Python layer
// captures the full loop into a single hipGraph.
#include <cmath>
#include <cstdlib>

#include "common.h"

namespace ldm {

// Layer index -> geometry.  0..8: enc1 enc2 enc3 enc4 bottleneck dec4 dec3 dec2 dec1 (model.py:178-194)
// 9..14: [CA2 q, CA2 kv, CA2 out, CA1 q, CA1 kv, CA1 out] 1x1 projections of the packed
// nn.MultiheadAttention in_proj / out_proj (model.py:132, :184-185).
static int layer_desc(const ldm_unet_shape& s, int layer, ldm_conv_desc& d) {
    LDM_REQUIRE(s.B > 0 && s.C > 0 && s.nf > 0, "unet: bad shape");
    LDM_REQUIRE(s.H % 8 == 0 && s.W % 8 == 0 && s.H >= 8 && s.W >= 8,
                "unet: latent H and W must be multiples of 8 (skip connections, model.py:221-227)");
    LDM_REQUIRE(s.nf * 4 == 256, "unet: CrossAttention dims are fixed at 512/256 (model.py:184-185) -> num_filters 64");
    d = ldm_conv_desc{};
    d.B = s.B;
    const int nf = s.nf;
    const int H = s.H, W = s.W;
    auto conv = [&](int cin, int hin, int win, int cout, int stride) {
        d.Cin = cin;
        d.Hin = hin;
        d.Win = win;
        d.Cout = cout;
        d.kh = d.kw = 3;
        d.stride = stride;
        d.pad = 1;
        d.out_pad = 0;
        d.transposed = 0;
        d.Hout = (hin + 2 - 3) / stride + 1;
        d.Wout = (win + 2 - 3) / stride + 1;
    };
    auto convT = [&](int cin, int hin, int win, int cout) {
        d.Cin = cin;
        d.Hin = hin;
        d.Win = win;
        d.Cout = cout;
        d.kh = d.kw = 3;
        d.stride = 2;
        d.pad = 1;
        d.out_pad = 1;
        d.transposed = 1;
        d.Hout = 2 * hin;
        d.Wout = 2 * win;
    };
    auto proj = [&](int cin, int cout, int hw) {
        d.Cin = cin;
        d.Hin = 1;
        d.Win = hw;
        d.Cout = cout;
        d.kh = d.kw = 1;
        d.stride = 1;
        d.pad = 0;
        d.out_pad = 0;
        d.transposed = 0;
        d.Hout = 1;
        d.Wout = hw;
    };
    const int L2 = (H / 4) * (W / 4), L1 = (H / 8) * (W / 8);
    switch (layer) {
        case 0: conv(s.C, H, W, nf, 1); break;
        case 1: conv(nf, H, W, 2 * nf, 2); break;
        case 2: conv(2 * nf, H / 2, W / 2, 4 * nf, 2); break;
        case 3: conv(4 * nf, H / 4, W / 4, 8 * nf, 2); break;
        case 4: conv(8 * nf, H / 8, W / 8, 8 * nf, 1); break;
        case 5: convT(8 * nf, H / 8, W / 8, 4 * nf); break;
        case 6: convT(4 * nf, H / 4, W / 4, 2 * nf); break;
        case 7: convT(2 * nf, H / 2, W / 2, nf); break;
        case 8: conv(nf, H, W, s.C, 1); break;
        case 9: proj(256, 256, L2); break;
        case 10: proj(256, 512, L2); break;
        case 11: proj(256, 256, L2); break;
        case 12: proj(512, 512, L1); break;
        case 13: proj(512, 1024, L1); break;
        case 14: proj(512, 512, L1); break;
        default: return fail(2, "unet: layer index out of range");
    }
    // Activation layouts inside the UNet: everything between the latent input (NCHW, read by enc1)
    // and the noise prediction (NCHW, written by dec1) is NHWC, so each K-chunk of an implicit-GEMM
    // operand is one 16-byte load per lane; the style-map K/V projections read the NCHW style maps and
    // stay channel-major (the attention reads K/V that way); q and the attention output are token-major.
    switch (layer) {
        case 0: d.layout = 2; break;           // z (NCHW) -> z1 (NHWC)
        case 8: d.layout = 1; break;           // d2 (NHWC) -> eps / fused update (NCHW)
        case 10: case 13: d.layout = 0; break; // s5 / s6 -> kv (channel-major)
        default: d.layout = 3; break;
    }
    return 0;
}

struct UNetWs {
    float *convws, *temb, *z1, *z2, *z3, *q2, *kv2, *a2, *c2, *z4, *q1, *kv1, *a1, *c1, *zb, *d4, *d3, *d2, *eps;
    float *kf2, *bf2, *kf1, *bf1;   // folded keys of both cross-attentions (reverse loop, use_fold)
    float* xs;                      // the sampler state in NHWC (reverse loop with the step kernels)
    float* uks;                     // split-K counters + slabs of the K-split step kernels (uconv.hip)
    float *ubn, *p1;                // the bottleneck's folded values U and CA1's probabilities (bfold.hip)
    // the guided loop (carved at twice the caller's batch): the base half's noise prediction, and the target and
    // base style maps / key biases side by side as one doubled batch
    float *eb, *s5cat, *s6cat, *kb5cat, *kb6cat;
    int64_t total;
};

// Largest split-K workspace over the 15 layers' plans (layers run one after another on one stream, so
// they share it; its counters are zero between launches).
static int64_t conv_ws_floats(const ldm_unet_weights* w) {
    if (!w) return 0;
    int64_t m = 0;
    for (int i = 0; i < 9; ++i) m = m > w->conv_plan[i].ws_floats ? m : w->conv_plan[i].ws_floats;
    for (int j = 0; j < 2; ++j) {
        m = m > w->ca_plan_q[j].ws_floats ? m : w->ca_plan_q[j].ws_floats;
        m = m > w->ca_plan_kv[j].ws_floats ? m : w->ca_plan_kv[j].ws_floats;
        m = m > w->ca_plan_o[j].ws_floats ? m : w->ca_plan_o[j].ws_floats;
    }
    return m;
}

// The reverse loop's bottleneck on CA1's folded values (bfold.hip) at the canonical plane, B <= 8.
static bool use_bneck_fold(const ldm_unet_shape& s, const ldm_unet_weights* w) {
    return w && w->use_fold && w->use_step && w->step_bneck_w && s.C == 32 && s.nf == 64 &&
           bneck_fold_supported(s.B, s.H, s.W);
}

// S5 / S6: key counts of CA2 / CA1 (style mixing: several references stacked along the keys); 0 = the map's own
// token count, which is every caller but a style mix.  Only the K/V projections and the folded keys scale.
// Invariant of the reverse loop's two phases (sample_prepare / sample_run): every region is a range of its own (take()
// never hands out overlapping ranges), and the regions the prepare phase fills (kv2, kv1, kf2, bf2, kf1, bf1, ubn,
// s5cat, s6cat, kb5cat, kb6cat, and behind the carve carve_sample's temb_all and temb_b) are written by no launch of
// the run phase, which writes z1 .. eps, q*, a*, c*, xs, p1, eb, carve_sample's keep region (kbase .. krows) and the two
// scratch regions.  Those two, convws and uks, are shared by both phases' launches (the K/V projections' split-K
// partials, the loop's) but carry nothing from one launch to the next beyond counters that are zero between launches.
// A region added for prepared data must keep to this: a range of its own that the loop does not write.
static UNetWs carve(const ldm_unet_shape& s, const ldm_unet_weights* wts, float* base, int64_t S5 = 0, int64_t S6 = 0,
                    bool guided = false) {
    const int64_t B = s.B, nf = s.nf, HW = (int64_t)s.H * s.W;
    const int64_t HW2 = HW / 4, L2 = HW / 16, L1 = HW / 64;
    if (S5 <= 0) S5 = L2;
    if (S6 <= 0) S6 = L1;
    UNetWs w{};
    int64_t off = 0;
    auto take = [&](int64_t n) {
        float* p = base ? base + off : nullptr;
        off += (n + 63) / 64 * 64;   // 256-byte aligned sub-buffers
        return p;
    };
    w.convws = take(conv_ws_floats(wts));   // first: the zero-filled counters live here
    w.temb = take(B * 128);
    w.z1 = take(B * nf * HW);
    w.z2 = take(B * 2 * nf * HW2);
    w.z3 = take(B * 4 * nf * L2);
    w.q2 = take(B * 256 * L2);
    w.kv2 = take(B * 512 * S5);
    w.a2 = take(B * 256 * L2);
    w.c2 = take(B * 256 * L2);
    w.z4 = take(B * 8 * nf * L1);
    w.q1 = take(B * 512 * L1);
    w.kv1 = take(B * 1024 * S6);
    w.a1 = take(B * 512 * L1);
    w.c1 = take(B * 512 * L1);
    w.zb = take(B * 8 * nf * L1);
    w.d4 = take(B * 4 * nf * L2);
    w.d3 = take(B * 2 * nf * HW2);
    w.d2 = take(B * nf * HW);
    w.eps = take(B * (int64_t)s.C * HW);
    w.kf2 = take(B * 4 * 256 * S5);
    w.bf2 = take(B * 4 * S5);
    w.kf1 = take(B * 4 * 512 * S6);
    w.bf1 = take(B * 4 * S6);
    w.xs = take(B * (int64_t)s.C * HW);
    w.uks = take(wts && wts->use_step ? step_ws_floats(s.B, s.H, s.W) : 0);
    const bool bfold = use_bneck_fold(s, wts) && S6 == L1;   // (its kernels are built for 16 keys)
    w.ubn = take(bfold ? B * 512 * 576 : 0);
    w.p1 = take(bfold ? B * 4 * L1 * L1 : 0);
    if (guided) {   // (after everything else: the unguided carve is the one it always was)
        w.eb = take(B / 2 * (int64_t)s.C * HW);
        w.s5cat = take(B * 256 * S5);
        w.s6cat = take(B * 512 * S6);
        w.kb5cat = take(B * S5);
        w.kb6cat = take(B * S6);
    }
    w.total = off;
    return w;
}

// The whole workspace of a reverse loop (ldm_sample_workspace_floats): the carve at the shape the body runs at and,
// behind it, unrounded and in this order, the regions below.  The one statement of that tail's layout.
struct SampleWs {
    ldm_unet_shape sh;   // the shape the body runs at: the caller's, guided at twice its batch (targets, then bases)
    UNetWs ws;
    // prepare phase: every step's time embeddings [nsteps * sh.B, 128]; guided, the caller's rows [nsteps * B, 128]
    float *temb_all, *temb_b;   // staged in temb_b before they are doubled into temb_all
    // run phase, only with the keep: the step kernels' keep region [e_b (guided)] [z0] [n0] [w] [rows].  kbase is its
    // start (e_b when guided, else z0); z0 / n0 in the state's NHWC layout; krows [nsteps, krl] = {a, b, scale[B] (guided)}
    float *kbase, *kz0, *kn0, *kw, *krows;
    int64_t krl, total;
};
static SampleWs carve_sample(const ldm_unet_shape& sc, const ldm_unet_weights* wts, float* base, int64_t S5, int64_t S6,
                             int64_t nsteps, bool guided, bool keep) {
    SampleWs w{};
    w.sh = sc, w.sh.B = guided ? 2 * sc.B : sc.B;
    w.ws = carve(w.sh, wts, base, S5, S6, guided);
    w.total = w.ws.total;
    auto take = [&](int64_t n) { return w.total += n, base ? base + (w.total - n) : nullptr; };
    const int64_t HW = (int64_t)sc.H * sc.W, dense = sc.B * sc.C * HW;
    w.temb_all = take(nsteps * w.sh.B * 128);
    w.temb_b = take(guided ? nsteps * sc.B * 128 : 0);
    w.krl = 2 + (guided ? sc.B : 0);
    if (keep) {
        w.kbase = take(guided ? dense : 0), w.kz0 = take(dense), w.kn0 = take(dense);
        w.kw = take(sc.B * HW), w.krows = take(nsteps * w.krl);
    }
    return w;
}

// Optional fusion of the reverse-loop update into dec1's epilogue (see EpiArgs::ddim_*).
struct DdimFuse {
    const float* coef;
    float eta;
    float* x;
    float* x0_log;
    float* eps_log;
    bool msolver;            // the multistep solver's update instead: coef is an 8-float row, eta unused, x0_log required
    const float* x0_prev;    // msolver: the previous step's x0 log or NULL (first-order step)
    // style guidance: gB = the caller's batch (the body runs at 2 gB: targets, then bases), 0 = none.  dec1 then runs
    // as two launches at gB: the base half as a plain conv into eb, the target half guided against it by gscale [gB],
    // updating x's first half and storing the new state to its second half too (x is the doubled state).
    int gB;
    float* eb;
    const float* gscale;
    // regional keep (keep_blend behind the update), kw == NULL: none.  conv.hip's loops read the caller's NCHW z0 / n0
    // and [B, H, W] weights with the step's row kcoef = {a, b}; the step kernels read the loop's keep region kbase
    // ([z0 | n0 | w], NHWC, led by e_b when guided: eb == kbase) and the step's row krow ({a, b}, then the strengths)
    const float *kz0, *kn0, *kw, *kcoef;
    const float *kbase, *krow;
    int64_t kstride;   // floats between the region's parts
};

// dec1's epilogue with the update fused in: the solver's row, the state, the logs and the keep
static void fuse_epi(EpiArgs& ep, const DdimFuse& fuse) {
    if (fuse.msolver) ep.ms_coef = fuse.coef, ep.ms_x0_prev = fuse.x0_prev;
    else ep.ddim_coef = fuse.coef;
    ep.ddim_eta = fuse.eta;
    ep.ddim_x = fuse.x;
    ep.ddim_x0_log = fuse.x0_log;
    ep.ddim_eps_log = fuse.eps_log;
    if (fuse.kw) ep.keep_z0 = fuse.kz0, ep.keep_n0 = fuse.kn0, ep.keep_w = fuse.kw, ep.keep_coef = fuse.kcoef;
}

static int conv_call(const ldm_unet_shape& s, float* convws, int layer, const ldm_conv_plan& plan, const float* x, const float* w,
                     const float* bias, int act, const float* bcast, const float* skip, float* y, hipStream_t st,
                     const DdimFuse* fuse = nullptr, const float* pos_bias = nullptr) {
    ldm_conv_desc d;
    int rc = layer_desc(s, layer, d);
    if (rc) return rc;
    EpiArgs ep{};
    ep.bias = pos_bias ? nullptr : bias;
    ep.pos_bias = pos_bias;
    ep.act = act;
    ep.bcast = bcast;
    ep.skip = skip;
    if (fuse) fuse_epi(ep, *fuse);
    return conv_forward_ex(d, plan, x, w, ep, y, convws, st);
}

#define LDM_TRY(expr)            \
    do {                         \
        int _rc = (expr);        \
        if (_rc) return _rc;     \
    } while (0)

// dec1 of conv.hip's loops: one launch with the fused update, or the guided loop's two at the caller's batch.  The
// bound plan is the doubled batch's; the halves run the same kind, tile and K split (the pack and the per-element
// summation order depend on nothing else), whose workspace need is no larger.
static int dec1_call(const ldm_unet_shape& s, const ldm_unet_weights& w, const float* d2, float* convws, float* out,
                     hipStream_t st, const DdimFuse* fuse) {
    if (!fuse || !fuse->gB)
        return conv_call(s, convws, 8, w.conv_plan[8], d2, w.conv_w[8], w.conv_b[8], LDM_ACT_NONE, nullptr, nullptr, out, st,
                         fuse);
    ldm_unet_shape sh = s;
    sh.B = fuse->gB;
    ldm_conv_desc d;
    LDM_TRY(layer_desc(sh, 8, d));
    const ldm_conv_plan& bound = w.conv_plan[8];
    LDM_REQUIRE(bound.kind >= 0 && bound.kind <= 2, "guided loop: dec1's plan must be a direct or fp32 MFMA plan");
    ldm_conv_plan plan;
    LDM_TRY(ldm_conv_make_plan_forced(&d, bound.kind, bound.tm, bound.tn, bound.wk, bound.balance ? -bound.ks : bound.ks, &plan));
    LDM_REQUIRE(plan.packed_floats == bound.packed_floats && plan.ws_floats <= bound.ws_floats, "guided loop: dec1 plan mismatch");
    const int64_t HW = (int64_t)s.H * s.W;
    EpiArgs eb{};
    eb.bias = w.conv_b[8];
    eb.act = LDM_ACT_NONE;
    LDM_TRY(conv_forward_ex(d, plan, d2 + fuse->gB * HW * s.nf, w.conv_w[8], eb, fuse->eb, convws, st));
    EpiArgs ep = eb;
    fuse_epi(ep, *fuse);
    ep.guide_eb = fuse->eb;
    ep.guide_scale = fuse->gscale;
    ep.ddim_x2 = fuse->x + fuse->gB * HW * s.C;
    return conv_forward_ex(d, plan, d2, w.conv_w[8], ep, nullptr, convws, st);
}

// K/V projections of the style maps (the key/value half of both cross-attentions' in_proj,
// model.py:153).  They depend only on s5 / s6, which are fixed for a whole reverse loop.
static int style_kv(const ldm_unet_shape& s, const ldm_unet_weights& w, const float* s5, const float* s6,
                    const UNetWs& ws, hipStream_t st) {
    LDM_TRY(conv_call(s, ws.convws, 10, w.ca_plan_kv[0], s5, w.ca_wkv[0], w.ca_bkv[0], 0, nullptr, nullptr, ws.kv2, st));
    LDM_TRY(conv_call(s, ws.convws, 13, w.ca_plan_kv[1], s6, w.ca_wkv[1], w.ca_bkv[1], 0, nullptr, nullptr, ws.kv1, st));
    return 0;
}

// One K/V projection over S style tokens instead of the map's own count (style mixing).  The weights are packed
// for the bound plan, and the pack depends on the plan's kernel kind and tile only, never on the token count:
// the same kind and tile are forced for the longer row, without a K split (no workspace beyond the bound one).
static int style_kv_tokens(const ldm_unet_shape& s, const ldm_unet_weights& w, int j, const float* sm, int S, float* kv,
                           hipStream_t st) {
    ldm_conv_desc d;
    LDM_TRY(layer_desc(s, 10 + 3 * j, d));
    d.Win = d.Wout = S;
    const ldm_conv_plan& bound = w.ca_plan_kv[j];
    LDM_REQUIRE(bound.kind >= 0 && bound.kind <= 2, "style mix: the K/V projection's plan must be a direct or fp32 MFMA plan");
    ldm_conv_plan plan;
    LDM_TRY(ldm_conv_make_plan_forced(&d, bound.kind, bound.tm, bound.tn, bound.wk, 1, &plan));
    LDM_REQUIRE(plan.packed_floats == bound.packed_floats && plan.ws_floats == 0, "style mix: K/V projection plan mismatch");
    EpiArgs ep{};
    ep.bias = w.ca_bkv[j];
    ep.act = 0;
    return conv_forward_ex(d, plan, sm, w.ca_wkv[j], ep, kv, nullptr, st);
}

// kv_ready: ws.kv2 / ws.kv1 already hold style_kv() of these s5 / s6 (the reverse loop computes them
// once, before its first step — the same kernel on the same inputs, so bitwise what each step's
// in-loop projection would produce).
static int unet_forward(const ldm_unet_shape& s, const ldm_unet_weights& w, const float* z, const void* t,
                        int t_is_float, const float* s5, const float* s6, float* out, const UNetWs& ws,
                        hipStream_t st, const float* temb_pre = nullptr, const DdimFuse* fuse = nullptr,
                        bool kv_ready = false) {
    const int HW = s.H * s.W;
    const int L2 = HW / 16, L1 = HW / 64;
    // t_embedding = time_mlp(t)[:, :, None, None]                               (model.py:203)
    const float* temb = temb_pre;
    if (!temb) {
        LDM_TRY(ldm_time_mlp_forward(t, t_is_float, s.B, 128, w.t_freqs, w.t_w1, w.t_b1, w.t_w2, w.t_b2, ws.temb, st));
        temb = ws.temb;
    }
    // z1 = relu(enc1(z)); z2 = relu(enc2(z1)) + t_emb; z3 = relu(enc3(z2))      (model.py:205-209)
    LDM_TRY(conv_call(s, ws.convws, 0, w.conv_plan[0], z, w.conv_w[0], w.conv_b[0], LDM_ACT_RELU, nullptr, nullptr, ws.z1, st));
    LDM_TRY(conv_call(s, ws.convws, 1, w.conv_plan[1], ws.z1, w.conv_w[1], w.conv_b[1], LDM_ACT_RELU, temb, nullptr, ws.z2, st));
    LDM_TRY(conv_call(s, ws.convws, 2, w.conv_plan[2], ws.z2, w.conv_w[2], w.conv_b[2], LDM_ACT_RELU, nullptr, nullptr, ws.z3, st));
    // z3 = cross_attention2(z3, s5)                                              (model.py:211)
    if (!kv_ready) LDM_TRY(style_kv(s, w, s5, s6, ws, st));
    LDM_TRY(conv_call(s, ws.convws, 9, w.ca_plan_q[0], ws.z3, w.ca_wq[0], w.ca_bq[0], 0, nullptr, nullptr, ws.q2, st));
    LDM_TRY(attention_core_ex(ws.q2, ws.kv2, ws.a2, s.B, 256, 4, L2, L2, (float)std::sqrt(1.0 / 64.0), true, st));
    LDM_TRY(conv_call(s, ws.convws, 11, w.ca_plan_o[0], ws.a2, w.ca_wo[0], w.ca_bo[0], 0, nullptr, nullptr, ws.c2, st));
    // z4 = relu(enc4(z3)); z4 = cross_attention1(z4, s6)                         (model.py:212-214)
    LDM_TRY(conv_call(s, ws.convws, 3, w.conv_plan[3], ws.c2, w.conv_w[3], w.conv_b[3], LDM_ACT_RELU, nullptr, nullptr, ws.z4, st));
    LDM_TRY(conv_call(s, ws.convws, 12, w.ca_plan_q[1], ws.z4, w.ca_wq[1], w.ca_bq[1], 0, nullptr, nullptr, ws.q1, st));
    LDM_TRY(attention_core_ex(ws.q1, ws.kv1, ws.a1, s.B, 512, 4, L1, L1, (float)std::sqrt(1.0 / 128.0), true, st));
    LDM_TRY(conv_call(s, ws.convws, 14, w.ca_plan_o[1], ws.a1, w.ca_wo[1], w.ca_bo[1], 0, nullptr, nullptr, ws.c1, st));
    // bottleneck + decoder with skips (ReLU before the add)                     (model.py:217-229)
    LDM_TRY(conv_call(s, ws.convws, 4, w.conv_plan[4], ws.c1, w.conv_w[4], w.conv_b[4], LDM_ACT_RELU, nullptr, nullptr, ws.zb, st));
    LDM_TRY(conv_call(s, ws.convws, 5, w.conv_plan[5], ws.zb, w.conv_w[5], w.conv_b[5], LDM_ACT_RELU, nullptr, ws.z3, ws.d4, st));
    LDM_TRY(conv_call(s, ws.convws, 6, w.conv_plan[6], ws.d4, w.conv_w[6], w.conv_b[6], LDM_ACT_RELU, nullptr, ws.z2, ws.d3, st));
    LDM_TRY(conv_call(s, ws.convws, 7, w.conv_plan[7], ws.d3, w.conv_w[7], w.conv_b[7], LDM_ACT_RELU, nullptr, ws.z1, ws.d2, st));
    LDM_TRY(dec1_call(s, w, ws.d2, ws.convws, out, st, fuse));
    return 0;
}

// The style map of a loop: per-(query position, reference) biases of CA2 / CA1 ([Bm,L2,R] / [Bm,L1,R], the caller's
// buffers), read by each step's two attentions (attention_folded_keys_map).  NULL: the launches are the key-bias ones.
struct RefBias {
    const float *b5, *b6;
    int R, Bm;   // references; samples that take the bias (guided: the target half)
};
// CA2 (j = 0) / CA1 (j = 1) of a folded step
static int step_attention(int j, const float* z, const float* kv, const float* kf, const float* bf, float* out, int B, int L,
                          int S, const RefBias* rb, hipStream_t st) {
    const int E = j ? 512 : 256;
    if (!rb) return attention_folded_keys(z, kv, kf, bf, nullptr, out, B, E, 4, L, S, st);
    return attention_folded_keys_map(z, kv, kf, bf, nullptr, j ? rb->b6 : rb->b5, rb->R, rb->Bm, out, B, E, 4, L, S, st);
}

// The reverse loop's step with both cross-attentions re-associated (style and weights are fixed for the
// whole loop): the Q in-projection folds into the keys (ldm_attention_fold_keys, once per loop) and the
// out-projection into the following conv (ldm_fold_conv_proj, once per weight version).  11 launches per
// step instead of 15; the same arithmetic up to fp32 re-association.
static int unet_forward_folded(const ldm_unet_shape& s, const ldm_unet_weights& w, const float* z, const UNetWs& ws,
                               hipStream_t st, const float* temb, const DdimFuse* fuse, int S5, int S6,
                               const RefBias* rb) {
    const int HW = s.H * s.W;
    const int L2 = HW / 16, L1 = HW / 64;
    LDM_TRY(conv_call(s, ws.convws, 0, w.conv_plan[0], z, w.conv_w[0], w.conv_b[0], LDM_ACT_RELU, nullptr, nullptr, ws.z1, st));
    LDM_TRY(conv_call(s, ws.convws, 1, w.conv_plan[1], ws.z1, w.conv_w[1], w.conv_b[1], LDM_ACT_RELU, temb, nullptr, ws.z2, st));
    LDM_TRY(conv_call(s, ws.convws, 2, w.conv_plan[2], ws.z2, w.conv_w[2], w.conv_b[2], LDM_ACT_RELU, nullptr, nullptr, ws.z3, st));
    // cross_attention2 then enc4 (model.py:211-212)
    LDM_TRY(step_attention(0, ws.z3, ws.kv2, ws.kf2, ws.bf2, ws.a2, s.B, L2, S5, rb, st));
    LDM_TRY(conv_call(s, ws.convws, 3, w.conv_plan[3], ws.a2, w.fold_w[0], nullptr, LDM_ACT_RELU, nullptr, nullptr, ws.z4, st,
                      nullptr, w.fold_pb[0]));
    // cross_attention1 then bottleneck (model.py:214-217)
    LDM_TRY(step_attention(1, ws.z4, ws.kv1, ws.kf1, ws.bf1, ws.a1, s.B, L1, S6, rb, st));
    LDM_TRY(conv_call(s, ws.convws, 4, w.conv_plan[4], ws.a1, w.fold_w[1], nullptr, LDM_ACT_RELU, nullptr, nullptr, ws.zb, st,
                      nullptr, w.fold_pb[1]));
    LDM_TRY(conv_call(s, ws.convws, 5, w.conv_plan[5], ws.zb, w.conv_w[5], w.conv_b[5], LDM_ACT_RELU, nullptr, ws.z3, ws.d4, st));
    LDM_TRY(conv_call(s, ws.convws, 6, w.conv_plan[6], ws.d4, w.conv_w[6], w.conv_b[6], LDM_ACT_RELU, nullptr, ws.z2, ws.d3, st));
    LDM_TRY(conv_call(s, ws.convws, 7, w.conv_plan[7], ws.d3, w.conv_w[7], w.conv_b[7], LDM_ACT_RELU, nullptr, ws.z1, ws.d2, st));
    LDM_TRY(dec1_call(s, w, ws.d2, ws.convws, nullptr, st, fuse));
    return 0;
}

// The same folded step on the step kernels (uconv.hip): x and every activation NHWC, 11 launches, the
// DDIM update fused into dec1.  z (the sampler state) is ws.xs.
static int unet_step_kernels(const ldm_unet_shape& s, const ldm_unet_weights& w, const UNetWs& ws, hipStream_t st,
                             const float* temb, const DdimFuse& fuse, int S5, int S6, bool bfold, const RefBias* rb) {
    const int HW = s.H * s.W;
    const int L2 = HW / 16, L1 = HW / 64;
    // the nine convs' operands: enc1..enc3, enc4 (after CA2), bottleneck (after CA1), dec4..dec2, dec1 + DDIM
    const float* xin[9] = {ws.xs, ws.z1, ws.z2, ws.a2, ws.a1, ws.zb, ws.d4, ws.d3, ws.d2};
    float* yout[9] = {ws.z1, ws.z2, ws.z3, ws.z4, ws.zb, ws.d4, ws.d3, ws.d2, nullptr};
    const float* bias[9] = {w.conv_b[0], w.conv_b[1], w.conv_b[2], w.step_pb[0], w.step_pb[1], w.conv_b[5], w.conv_b[6],
                            w.conv_b[7], w.conv_b[8]};
    const float* skip[9] = {nullptr, nullptr, nullptr, nullptr, nullptr, ws.z3, ws.z2, ws.z1, nullptr};
    StepConv c[9];
    for (int l = 0; l < 9; ++l) {
        c[l] = StepConv{};
        c[l].x = xin[l];
        c[l].w = w.step_w[l];
        c[l].y = yout[l];
        c[l].bias = bias[l];
        c[l].skip = skip[l];
        c[l].dtype = w.step_dtype;
        c[l].ws = ws.uks;
    }
    c[1].bcast = temb;
    c[8].coef = fuse.coef;
    c[8].eta = fuse.eta;
    c[8].xs = ws.xs;
    c[8].x0_log = fuse.x0_log;
    c[8].eps_log = fuse.eps_log;
    c[8].msolver = fuse.msolver;
    c[8].x0_prev = fuse.x0_prev;
    if (fuse.kw && !fuse.gB) c[8].keep_base = fuse.kbase, c[8].keep_row = fuse.krow, c[8].keep_stride = fuse.kstride;
    auto dec1_guided = [&]() -> int {   // the base half into eb, then the target half guided against it
        const int Bh = fuse.gB;
        StepConv cb = c[8];
        cb.x = ws.d2 + (size_t)Bh * HW * s.nf;
        cb.y = fuse.eb;
        cb.plain = 1;
        cb.coef = nullptr, cb.xs = nullptr, cb.x0_log = nullptr, cb.eps_log = nullptr, cb.msolver = 0, cb.x0_prev = nullptr;
        LDM_TRY(step_conv(8, Bh, s.H, s.W, cb, st));
        StepConv ct = c[8];
        ct.guide_eb = fuse.eb;
        ct.guide_scale = fuse.gscale;
        ct.xs2 = ws.xs + (size_t)Bh * HW * s.C;
        if (fuse.kw)   // (eb == kbase)
            ct.keep_base = fuse.kbase, ct.keep_row = fuse.krow, ct.keep_stride = fuse.kstride, ct.guide_scale = nullptr;
        return step_conv(8, Bh, s.H, s.W, ct, st);
    };
    auto run = [&](int l0, int l1) -> int {   // layers [l0, l1]
        for (int l = l0; l <= l1; ++l) {
            if (l == 8 && fuse.gB) LDM_TRY(dec1_guided());
            else LDM_TRY(step_conv(l, s.B, s.H, s.W, c[l], st));
        }
        return 0;
    };
    LDM_TRY(run(0, 2));
    LDM_TRY(step_attention(0, ws.z3, ws.kv2, ws.kf2, ws.bf2, ws.a2, s.B, L2, S5, rb, st));
    LDM_TRY(run(3, 3));
    if (bfold) {
        // CA1's probabilities, then the bottleneck on its folded values U (formed before the loop)
        if (ca1_probs_own()) LDM_TRY(ca1_probs(ws.z4, ws.kf1, ws.bf1, ws.p1, s.B, ca1_keys_packed(), st));
        else LDM_TRY(attention_folded_probs(ws.z4, ws.kf1, ws.bf1, ws.p1, s.B, 512, 4, L1, L1, st));
        LDM_TRY(bneck_pv(ws.ubn, ws.p1, w.step_pb[1], ws.zb, s.B, w.step_dtype, st));
        return run(5, 8);
    }
    LDM_TRY(step_attention(1, ws.z4, ws.kv1, ws.kf1, ws.bf1, ws.a1, s.B, L1, S6, rb, st));
    return run(4, 8);
}

}  // namespace ldm

using namespace ldm;

extern "C" int ldm_step_layer_forms(int32_t* ks_layers) {
    LDM_REQUIRE(ks_layers, "step_layer_forms: null argument");
    *ks_layers = step_ks_mask();   // (their K-split geometry: LDM_UCONV_KS2, uconv.hip kKs2)
    return 0;
}

extern "C" int ldm_unet_layer_desc(const ldm_unet_shape* s, int32_t layer, ldm_conv_desc* d) {
    LDM_REQUIRE(s && d, "unet_layer_desc: null argument");
    return layer_desc(*s, layer, *d);
}

extern "C" int64_t ldm_unet_workspace_floats(const ldm_unet_shape* s, const ldm_unet_weights* w) {
    if (!s) return -1;
    return carve(*s, w, nullptr).total;
}

extern "C" int ldm_unet_make_plans(const ldm_unet_shape* s, ldm_unet_weights* w) {
    LDM_REQUIRE(s && w, "unet_make_plans: null argument");
    for (int l = 0; l < 15; ++l) {
        ldm_conv_desc d;
        LDM_TRY(layer_desc(*s, l, d));
        ldm_conv_plan* p = l < 9 ? &w->conv_plan[l]
                                 : ((l - 9) % 3 == 0 ? &w->ca_plan_q[(l - 9) / 3]
                                                     : ((l - 9) % 3 == 1 ? &w->ca_plan_kv[(l - 9) / 3]
                                                                         : &w->ca_plan_o[(l - 9) / 3]));
        LDM_TRY(ldm_conv_make_plan(&d, p));
    }
    return 0;
}

extern "C" int ldm_unet_forward(const ldm_unet_shape* s, const ldm_unet_weights* w, const float* z, const void* t,
                                int32_t t_is_float, const float* s5, const float* s6, float* out, float* workspace,
                                void* stream) {
    LDM_REQUIRE(s && w && z && t && s5 && s6 && out && workspace, "unet_forward: null argument");
    UNetWs ws = carve(*s, w, workspace);
    return unet_forward(*s, *w, z, t, t_is_float, s5, s6, out, ws, (hipStream_t)stream);
}

// The reverse loop of both samplers.  msolver: coef_table is [nsteps, 8] (multistep rows) and every step i > 0 reads
// step i-1's slot of x0_logs as its history (a first-order row there carries c_1 = 0); step 0 has none to read.
// Style mixing (S5 / S6 > 0 and key_bias5 / key_bias6): s5 / s6 hold S5 / S6 style tokens per
// sample, the K/V projections and the key fold run over them, the bias goes into the folded keys' bias, and the
// two attention launches of each step stream the keys (stylemix.hip).  With the maps' own counts and no bias every
// call below is the one it always was.
// Style map (ref_bias5 / ref_bias6 with refs): the weight of each stacked reference per query position.  It has a query
// axis, so it cannot go into bf: each step's two attention launches read it (attention_folded_keys_map), and the
// prepare phase does not.  Guided, it applies to the target half only (Bm = the caller's batch).
// Style guidance (g != NULL): every step evaluates the denoiser under the target and under a
// base style and steps on eps = e_b + scale (e_t - e_b) (guide_eps).  The body runs at twice the caller's batch,
// samples [0, B) under the target maps and [B, 2B) under the base maps, on a doubled sampler state whose halves
// stay bitwise equal; w holds the doubled batch's plans.  Only dec1 differs (dec1_call / unet_step_kernels).
struct Guide {
    const float *s5_base, *s6_base, *key_bias5_base, *key_bias6_base, *scale;
};
// The regional keep (k != NULL): after every step's update the state is blended with the content's
// own noising trajectory coef[i][0] z0 + coef[i][1] n0 under the keep weights w [B, H, W] (keep_blend); the logs and
// the 2M history stay the model's prediction.  Only dec1's epilogue differs.  The step kernels read z0 / n0 in the
// state's NHWC layout from a keep region behind the time embeddings (carve_sample), filled once per loop.
struct Keep {
    const float *z0, *n0, *w, *coef;
};
// rows[i] = {coef[i][0], coef[i][1], scale[0 .. B)} (scale NULL: rows of two)
__global__ __launch_bounds__(256) void keep_rows_kernel(const float* __restrict__ coef, const float* __restrict__ scale,
                                                        float* __restrict__ rows, int B, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over rows
    if (i >= n) return;
    const int rl = 2 + (scale ? B : 0);
    const int64_t r = i / rl;
    const int j = (int)(i - r * rl);
    rows[i] = j < 2 ? coef[2 * r + j] : scale[j - 2];
}

// out[r] = a[r] ++ b[r] for rows of rowlen floats (NULL a / b: zeros): the doubled batch's operands, once per loop
__global__ __launch_bounds__(256) void concat_halves_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                            float* __restrict__ out, int64_t rowlen, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over out
    if (i >= n) return;
    const int64_t r = i / (2 * rowlen), j = i - r * 2 * rowlen;
    const float* src = j < rowlen ? a : b;
    out[i] = src ? src[r * rowlen + (j < rowlen ? j : j - rowlen)] : 0.f;
}
static int concat_halves(const float* a, const float* b, float* out, int64_t rows, int64_t rowlen, hipStream_t st) {
    const int64_t n = rows * 2 * rowlen;
    hipLaunchKernelGGL(concat_halves_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, b, out, rowlen, n);
    LDM_CHECK_LAUNCH("concat_halves_kernel");
    return 0;
}

// What both phases of the loop derive from one set of arguments: the shape the body runs at, the key counts, the
// workspace's regions and which forms apply.  loop_plan makes the checks that do not depend on the phase, so that
// the prepare and the run refuse the same arguments.
struct LoopPlan {
    int S5, S6;           // key counts of CA2 / CA1
    bool kb5, kb6;        // a key bias reaches the folded keys (guided: the target's or the base's)
    bool bfold;           // the bottleneck runs on CA1's folded values
    bool map;             // a style map: each step's two attentions read the reference biases (run phase only)
    RefBias rb;
    SampleWs sw;          // the workspace's regions and the shape the body runs at
    int64_t dense;        // one step of the logs: the caller's batch
};
static int loop_plan(const ldm_unet_shape* sc, const ldm_unet_weights* w, const ldm_sample_args& a, const Guide* g,
                     bool keep, LoopPlan& lp) {
    const int L2 = sc->H * sc->W / 16, L1 = sc->H * sc->W / 64;
    lp.S5 = a.S5 <= 0 ? L2 : a.S5;
    lp.S6 = a.S6 <= 0 ? L1 : a.S6;
    lp.kb5 = a.key_bias5 || (g && g->key_bias5_base);
    lp.kb6 = a.key_bias6 || (g && g->key_bias6_base);
    const bool mix = lp.S5 != L2 || lp.S6 != L1 || lp.kb5 || lp.kb6;
    LDM_REQUIRE(!mix || w->use_fold, "style mix: the reverse loop attends over several references only with the "
                                     "folded cross-attentions (use_fold)");
    lp.map = a.ref_bias5 != nullptr;
    lp.rb = RefBias{a.ref_bias5, a.ref_bias6, a.refs, sc->B};
    if (lp.map) {
        LDM_REQUIRE(w->use_fold, "style map: the reverse loop takes per-position reference weights only with the "
                                 "folded cross-attentions (use_fold)");
        LDM_REQUIRE((int64_t)a.refs * L2 == lp.S5 && (int64_t)a.refs * L1 == lp.S6,
                    "style map: S5 / S6 must be refs times the maps' own token counts");
    }
    lp.sw = carve_sample(*sc, w, a.workspace, lp.S5, lp.S6, a.nsteps, g != nullptr, keep);
    lp.dense = (int64_t)sc->B * sc->C * sc->H * sc->W;
    LDM_REQUIRE(a.log_step_stride == 0 || a.log_step_stride >= lp.dense, "ddim_sample: log stride smaller than a step");
    if (w->use_fold) {
        LDM_REQUIRE(w->ca_wq_raw[0] && w->ca_wq_raw[1] && w->fold_w[0] && w->fold_w[1] && w->fold_pb[0] && w->fold_pb[1],
                    "ddim_sample: use_fold needs the folded weights");
        if (w->use_step) {
            LDM_REQUIRE(sc->C == 32 && sc->nf == 64, "ddim_sample: the step kernels are built for latent 32 / 64 filters");
            for (int l = 0; l < 9; ++l) LDM_REQUIRE(w->step_w[l], "ddim_sample: use_step needs the step weights");
            LDM_REQUIRE(w->step_pb[0] && w->step_pb[1], "ddim_sample: use_step needs the folded biases");
            LDM_REQUIRE(w->step_dtype >= LDM_DT_F32 && w->step_dtype <= LDM_DT_BF16, "ddim_sample: step_dtype");
            // the bottleneck's value fold is built for CA1's own 16 keys without a bias: a mix leaves it
            lp.bfold = use_bneck_fold(lp.sw.sh, w) && lp.S6 == L1 && !lp.kb6 && !lp.map;   // (nor does a style map)
        }
    }
    return 0;
}

// The prepare phase: everything that reads only the style maps, the key biases, the t table and the weights, never
// the sampler state, the logs, the coefficient table, the keep operands or the style map's reference biases (lp.rb is
// not touched here: any number of runs with other biases may follow).  It fills temb_all, the *cat buffers,
// kv2 / kv1, kf* / bf* and ubn, which the run phase only reads (the invariant stated on carve).
static int sample_prepare(const ldm_unet_shape* sc, const ldm_unet_weights* w, const ldm_sample_args& a, const Guide* g,
                          const LoopPlan& lp) {
    const ldm_unet_shape* s = &lp.sw.sh;
    const UNetWs& ws = lp.sw.ws;
    const int L2 = s->H * s->W / 16, L1 = s->H * s->W / 64;
    const int32_t nsteps = a.nsteps, S5 = lp.S5, S6 = lp.S6;
    const float *s5 = a.s5, *s6 = a.s6, *key_bias5 = a.key_bias5, *key_bias6 = a.key_bias6;
    float *temb_all = lp.sw.temb_all, *temb_b = lp.sw.temb_b;
    hipStream_t st = (hipStream_t)a.stream;
    // The time MLP depends only on t: all nsteps*B embeddings in one launch before the loop (the same
    // evaluations the reference makes one step at a time, model.py:203).
    LDM_TRY(ldm_time_mlp_forward(a.t_table, 0, nsteps * sc->B, 128, w->t_freqs, w->t_w1, w->t_b1, w->t_w2, w->t_b2,
                                 g ? temb_b : temb_all, st));
    if (g) {   // both halves share t: the caller's [nsteps, B] rows, each repeated for the base half
        LDM_TRY(concat_halves(temb_b, temb_b, temb_all, nsteps, (int64_t)sc->B * 128, st));
        // the doubled batch's style maps and key biases: targets, then bases
        LDM_TRY(concat_halves(s5, g->s5_base, ws.s5cat, 1, (int64_t)sc->B * 256 * S5, st));
        LDM_TRY(concat_halves(s6, g->s6_base, ws.s6cat, 1, (int64_t)sc->B * 512 * S6, st));
        s5 = ws.s5cat, s6 = ws.s6cat;
        if (key_bias5 || g->key_bias5_base) {
            LDM_TRY(concat_halves(key_bias5, g->key_bias5_base, ws.kb5cat, 1, (int64_t)sc->B * S5, st));
            key_bias5 = ws.kb5cat;
        }
        if (key_bias6 || g->key_bias6_base) {
            LDM_TRY(concat_halves(key_bias6, g->key_bias6_base, ws.kb6cat, 1, (int64_t)sc->B * S6, st));
            key_bias6 = ws.kb6cat;
        }
    }
    // Likewise the style maps' K/V projections (model.py:153 with kv = s5 / s6, fixed for the loop).
    if (S5 == L2 && S6 == L1) {
        LDM_TRY(style_kv(*s, *w, s5, s6, ws, st));
    } else {
        LDM_TRY(style_kv_tokens(*s, *w, 0, s5, S5, ws.kv2, st));
        LDM_TRY(style_kv_tokens(*s, *w, 1, s6, S6, ws.kv1, st));
    }
    if (w->use_fold) {
        LDM_TRY(attention_fold_keys_bias(ws.kv2, w->ca_wq_raw[0], w->ca_bq[0], s->B, 256, 4, S5,
                                         (float)std::sqrt(1.0 / 64.0), key_bias5, ws.kf2, ws.bf2, st));
        // With the fold, kf1 holds CA1's keys in the packed order while ca1_keys_packed() (bfold.hip; the step's
        // ca1_probs asks the same question): folded in the plain layout into the head of ubn (U, not yet formed, is 18
        // times their size) and packed from there into kf1; U follows on the same stream.  The workspace keeps its size.
        const bool kpack = lp.bfold && ca1_keys_packed();
        LDM_TRY(attention_fold_keys_bias(ws.kv1, w->ca_wq_raw[1], w->ca_bq[1], s->B, 512, 4, S6,
                                         (float)std::sqrt(1.0 / 128.0), key_bias6, kpack ? ws.ubn : ws.kf1, ws.bf1, st));
        if (kpack) LDM_TRY(ca1_pack_keys(ws.ubn, ws.kf1, s->B, st));
        if (lp.bfold) LDM_TRY(bneck_fold_values(w->step_bneck_w, ws.kv1, ws.ubn, s->B, st));
    }
    return 0;
}

// The run phase: the sampler state in and out, the keep region's fill and the loop itself, on a workspace that
// sample_prepare has filled for the same shape, weights and arguments.  It writes none of the prepared regions.
static int sample_run(const ldm_unet_shape* sc, const ldm_unet_weights* w, const ldm_sample_args& a, const Guide* g,
                      const Keep* kp, const LoopPlan& lp) {
    const ldm_unet_shape* s = &lp.sw.sh;
    const SampleWs& sw = lp.sw;
    const UNetWs& ws = sw.ws;
    const bool msolver = a.solver == LDM_SOLVER_MULTISTEP;
    const int32_t nsteps = a.nsteps, S5 = lp.S5, S6 = lp.S6;
    const float eta = msolver ? 0.f : a.eta;
    float *x = a.x, *x0_logs = a.x0_logs, *eps_logs = a.eps_logs, *temb_all = sw.temb_all;
    const float* coef_table = a.coef_table;
    // the literal loop's unet_forward names the maps, but with kv_ready it reads only their prepared projections
    const float *s5 = g ? ws.s5cat : a.s5, *s6 = g ? ws.s6cat : a.s6;
    const int64_t dense = lp.dense, n = a.log_step_stride ? a.log_step_stride : dense;
    hipStream_t st = (hipStream_t)a.stream;
    const size_t cw = msolver ? 8 : 4;   // floats per coefficient row
    const int HW = s->H * s->W;
    const RefBias* rb = lp.map ? &lp.rb : nullptr;
    // Joint sampling (seam_cols > 0, B > 1): the batch rows are neighbouring windows, fused across their seams before
    // step 0 and after every step's update (seam.hip).  Guided, each half of the doubled state on its own.  Off, nothing
    // is launched and the loops below are the ones they always were.
    const int seam = sc->B > 1 ? a.seam_cols : 0;
    auto fuse_seams = [&](float* xstate, bool nhwc) -> int {
        return seam ? seam_fuse(xstate, g ? 2 : 1, sc->B, s->C, s->H, s->W, seam, nhwc, st) : 0;
    };
    auto make_fuse = [&](int i, float* xstate) {
        DdimFuse fuse{coef_table + cw * (size_t)i, eta, xstate, x0_logs ? x0_logs + (size_t)i * n : nullptr,
                      eps_logs ? eps_logs + (size_t)i * n : nullptr, msolver,
                      msolver && i > 0 ? x0_logs + (size_t)(i - 1) * n : nullptr};
        if (g) fuse.gB = sc->B, fuse.eb = ws.eb, fuse.gscale = g->scale;
        if (kp) fuse.kz0 = kp->z0, fuse.kn0 = kp->n0, fuse.kw = kp->w, fuse.kcoef = kp->coef + 2 * (size_t)i;
        return fuse;
    };
    if (w->use_fold && w->use_step) {
        LDM_TRY(step_layout(x, ws.xs, sc->B, s->C, HW, true, st));
        if (g) LDM_TRY(step_layout(x, ws.xs + dense, sc->B, s->C, HW, true, st));
        if (kp) {   // the keep region
            LDM_TRY(step_layout(kp->z0, sw.kz0, sc->B, s->C, HW, true, st));
            LDM_TRY(step_layout(kp->n0, sw.kn0, sc->B, s->C, HW, true, st));
            LDM_HIP_TRY(hipMemcpyAsync(sw.kw, kp->w, (size_t)sc->B * HW * 4, hipMemcpyDeviceToDevice, st));
            const int64_t nr = (int64_t)nsteps * sw.krl;
            hipLaunchKernelGGL(keep_rows_kernel, dim3((unsigned)((nr + 255) / 256)), dim3(256), 0, st, kp->coef,
                               g ? g->scale : nullptr, sw.krows, sc->B, nr);
            LDM_CHECK_LAUNCH("keep_rows_kernel");
        }
        LDM_TRY(fuse_seams(ws.xs, true));
        for (int i = 0; i < nsteps; ++i) {
            DdimFuse fuse = make_fuse(i, ws.xs);
            if (kp) {
                fuse.kbase = sw.kbase, fuse.krow = sw.krows + (size_t)i * sw.krl, fuse.kstride = dense;
                if (g) fuse.eb = sw.kbase;   // e_b leads the keep region
            }
            LDM_TRY(unet_step_kernels(*s, *w, ws, st, temb_all + (size_t)i * s->B * 128, fuse, S5, S6, lp.bfold, rb));
            LDM_TRY(fuse_seams(ws.xs, true));
        }
        return step_layout(ws.xs, x, sc->B, s->C, HW, false, st);
    }
    // conv.hip's loops keep the state NCHW: in place on x, or when guided on the doubled state in the workspace
    float* xstate = x;
    if (g) {
        LDM_TRY(concat_halves(x, x, ws.xs, 1, dense, st));
        xstate = ws.xs;
    }
    LDM_TRY(fuse_seams(xstate, false));
    for (int i = 0; i < nsteps; ++i) {
        // noise_pred = unet(x, t, style_embedding)                                (model.py:439)
        // and, fused into dec1's epilogue, the x0 / direction / eta update and the two log clones
        // (model.py:442-463) — bitwise the same fp32 op sequence as ldm_ddim_step.
        const DdimFuse fuse = make_fuse(i, xstate);
        if (w->use_fold)
            LDM_TRY(unet_forward_folded(*s, *w, xstate, ws, st, temb_all + (size_t)i * s->B * 128, &fuse, S5, S6, rb));
        else
            LDM_TRY(unet_forward(*s, *w, xstate, a.t_table + (size_t)i * sc->B, 0, s5, s6, nullptr, ws, st,
                                 temb_all + (size_t)i * s->B * 128, &fuse, /*kv_ready=*/true));
        LDM_TRY(fuse_seams(xstate, false));
    }
    if (g) LDM_HIP_TRY(hipMemcpyAsync(x, ws.xs, (size_t)dense * 4, hipMemcpyDeviceToDevice, st));
    return 0;
}

// ---- the one sampler entry (ldm_capi.h ldm_sample_args) ----------------------------------------------------------
// An option is on when any of its pointers is set; ldm_sample then requires the rest of that group.
static bool guidance_on(const ldm_sample_args& a) { return a.s5_base || a.s6_base || a.guide_scale; }
static bool keep_on(const ldm_sample_args& a) { return a.z0 || a.n0 || a.keep || a.keep_coef; }

extern "C" int64_t ldm_sample_workspace_floats(const ldm_unet_shape* s, const ldm_unet_weights* w, const ldm_sample_args* a) {
    if (!s || !a || a->nsteps < 0 || a->S5 < 0 || a->S6 < 0 || s->B <= 0) return -1;
    return carve_sample(*s, w, nullptr, a->S5, a->S6, a->nsteps, guidance_on(*a), keep_on(*a)).total;
}

// The two scratch regions that hold split-K counters and must be zero before a launch: convws at the carve's start
// and uks, each with the size carve takes for it.  Everything else in the workspace is written before it is read.
extern "C" int ldm_sample_workspace_zeroed(const ldm_unet_shape* s, const ldm_unet_weights* w, const ldm_sample_args* a,
                                           int64_t* ranges) {
    LDM_REQUIRE(s && a && ranges && a->S5 >= 0 && a->S6 >= 0 && s->B > 0, "sample_workspace_zeroed: bad argument");
    float* const base = reinterpret_cast<float*>(uintptr_t(256));   // (only differences of the carved pointers are read)
    const SampleWs sw = carve_sample(*s, w, base, a->S5, a->S6, 0, guidance_on(*a), false);
    ranges[0] = sw.ws.convws - base;
    ranges[1] = conv_ws_floats(w);
    ranges[2] = sw.ws.uks - base;
    ranges[3] = w && w->use_step ? step_ws_floats(sw.sh.B, sw.sh.H, sw.sh.W) : 0;
    return 0;
}

// The struct carries no buffer size, and the sizes differ by more than a factor of two between configurations: a
// buffer sized for another one would be written past its end.  Before anything is launched the extent of the device
// allocation that holds `workspace` is asked of the runtime and compared with `need` floats.  This is exact for a
// buffer that is an allocation of its own; a buffer carved from a larger pool is only known to end inside the pool.
// Skipped under stream capture (a captured loop is run eagerly first) and where the runtime does not know the pointer.
static int workspace_extent_ok(int64_t need, const float* workspace, void* stream) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)stream, &cs) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    if (cs != hipStreamCaptureStatusNone) return 0;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)workspace) != hipSuccess || !base) {
        (void)hipGetLastError();
        return 0;
    }
    LDM_REQUIRE(need > 0, "sample: bad shape for the workspace size");
    const int64_t avail = (int64_t)(((const char*)base + size) - (const char*)workspace);
    LDM_REQUIRE(avail >= need * 4, "sample: the workspace's allocation ends before the size ldm_sample_workspace_floats "
                                   "gives for these arguments (was it sized for another configuration?)");
    return 0;
}

// The argument checks and the workspace-extent check of all three entries.  *skip: nothing to launch (nsteps == 0).
static int sample_check(const ldm_unet_shape* s, const ldm_unet_weights* w, const ldm_sample_args* a, bool* skip) {
    LDM_REQUIRE(s && w && a, "sample: null argument");
    LDM_REQUIRE(a->solver == LDM_SOLVER_DDIM || a->solver == LDM_SOLVER_MULTISTEP, "sample: unknown solver");
    const bool msolver = a->solver == LDM_SOLVER_MULTISTEP;
    LDM_REQUIRE(a->x && a->s5 && a->s6 && a->t_table && a->coef_table && a->workspace && (!msolver || a->x0_logs),
                "sample: null argument");
    LDM_REQUIRE(a->nsteps >= 0, "sample: negative step count");
    LDM_REQUIRE(a->S5 >= 0 && a->S6 >= 0, "sample: negative key count");
    LDM_REQUIRE(a->seam_cols >= 0 && a->seam_cols <= s->W / 2, "sample: seam_cols must lie in [0, W / 2]");
    const bool guided = guidance_on(*a), keep = keep_on(*a);
    if (guided) {
        LDM_REQUIRE(a->s5_base && a->s6_base, "guided sample: null base style maps");
        LDM_REQUIRE(a->guide_scale, "guided sample: null guidance scale");
        LDM_REQUIRE(s->B > 0 && s->B <= (1 << 20), "guided sample: bad batch");
    } else {
        LDM_REQUIRE(!a->key_bias5_base && !a->key_bias6_base, "sample: base key biases without a base style");
    }
    LDM_REQUIRE(!keep || (a->z0 && a->n0 && a->keep && a->keep_coef),
                "sample: z0, n0, keep and keep_coef go together (one is NULL)");
    LDM_REQUIRE((a->ref_bias5 != nullptr) == (a->ref_bias6 != nullptr),
                "sample: ref_bias5 and ref_bias6 go together (one is NULL)");
    LDM_REQUIRE(a->ref_bias5 ? a->refs >= 1 : a->refs == 0,
                "sample: refs is the reference count of ref_bias5 / ref_bias6 (at least 1 with them, 0 without)");
    *skip = a->nsteps == 0;
    if (*skip) return 0;
    return workspace_extent_ok(ldm_sample_workspace_floats(s, w, a), a->workspace, a->stream);
}

enum { PHASE_PREPARE = 1, PHASE_RUN = 2 };
static int sample_phases(const ldm_unet_shape* s, const ldm_unet_weights* w, const ldm_sample_args* a, int phases) {
    bool skip = false;
    LDM_TRY(sample_check(s, w, a, &skip));
    if (skip) return 0;
    const Guide g{a->s5_base, a->s6_base, a->key_bias5_base, a->key_bias6_base, a->guide_scale};
    const Keep k{a->z0, a->n0, a->keep, a->keep_coef};
    const Guide* gp = guidance_on(*a) ? &g : nullptr;
    LoopPlan lp{};
    LDM_TRY(loop_plan(s, w, *a, gp, keep_on(*a), lp));
    if (phases & PHASE_PREPARE) LDM_TRY(sample_prepare(s, w, *a, gp, lp));
    if (phases & PHASE_RUN) LDM_TRY(sample_run(s, w, *a, gp, keep_on(*a) ? &k : nullptr, lp));
    return 0;
}

extern "C" int ldm_sample_prepare(const ldm_unet_shape* s, const ldm_unet_weights* w, const ldm_sample_args* a) {
    return sample_phases(s, w, a, PHASE_PREPARE);
}
extern "C" int ldm_sample_run(const ldm_unet_shape* s, const ldm_unet_weights* w, const ldm_sample_args* a) {
    return sample_phases(s, w, a, PHASE_RUN);
}
// The prepare followed by the run: the launches ldm_sample always made, in the order it made them.
extern "C" int ldm_sample(const ldm_unet_shape* s, const ldm_unet_weights* w, const ldm_sample_args* a) {
    return sample_phases(s, w, a, PHASE_PREPARE | PHASE_RUN);
}
