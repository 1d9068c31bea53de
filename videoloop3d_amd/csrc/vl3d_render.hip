// C ABI of the fused MPI/MPV render (include/vl3d.h): argument checks, scratch layout and the dispatch to the convention that was
// compiled for (coord_mode, border_mode, act_order) -- one translation unit each, vl3d_render_c*.hip.  Kernels: vl3d_render_core.h.
//
// Replaces (reference, /root/reference): MPV.py:351-454 (planar geometry) ==
// utils_mpi.py:159-176 (warp_homography) + utils_mpi.py:92-107 (overcompose), and their autograd.
#include <string>
#include "vl3d_render_args.h"

using namespace vl3d_render_detail;

namespace {

// conventions a caller can reach (every other combination of the three enums returns VL3D_EUNSUPPORTED):
//   (UTILS_MPI, ZEROS,   PRE )  the reference's utils_mpi chain                       sigmoid/sigmoid, none/none, none/sigmoid
//   (AFFINE,    HARDCUT, POST)  the reference's MPV.py planar convention              all nine activation pairs
//   (AFFINE_PLANES, HARDCUT, POST)  MPV.py atlas-cell sampling: per-plane texel transform + quad extent   sigmoid/sigmoid
//   (UTILS_MPI, ZEROS,   POST), (UTILS_MPI, HARDCUT, PRE)  cross-check conventions     sigmoid/sigmoid
//   (AFFINE,    HARDCUT, BAKED) the planar convention under the bake rule: the picture the viewer package shows   sigmoid/sigmoid
typedef int (*ConvFn)(bool, const vl3d_render_desc *, const RenderArgs &, hipStream_t);
ConvFn conv_of(const vl3d_render_desc *d) {
    const int c = d->coord_mode, b = d->border_mode, o = d->act_order;
    if (c == VL3D_COORD_UTILS_MPI && b == VL3D_BORDER_ZEROS && o == VL3D_ACT_PRE) return conv_utils_zeros_pre;
    if (c == VL3D_COORD_UTILS_MPI && b == VL3D_BORDER_ZEROS && o == VL3D_ACT_POST) return conv_utils_zeros_post;
    if (c == VL3D_COORD_UTILS_MPI && b == VL3D_BORDER_HARDCUT && o == VL3D_ACT_PRE) return conv_utils_hardcut_pre;
    if (c == VL3D_COORD_AFFINE_PLANES && b == VL3D_BORDER_HARDCUT && o == VL3D_ACT_POST) return conv_affine_planes_hardcut_post;
    if (c == VL3D_COORD_AFFINE && b == VL3D_BORDER_HARDCUT && o == VL3D_ACT_POST)
        return (d->rgb_act == VL3D_ACT_SIGMOID && d->alpha_act == VL3D_ACT_SIGMOID) ? conv_affine_hardcut_post_sig : conv_affine_hardcut_post_other;
    if (o == VL3D_ACT_BAKED) {      // the bake rule: the planar MPV geometry with the shipped activations alone (no clip gradient for unbounded ones)
        if (c == VL3D_COORD_AFFINE && b == VL3D_BORDER_HARDCUT && d->rgb_act == VL3D_ACT_SIGMOID && d->alpha_act == VL3D_ACT_SIGMOID)
            return conv_affine_hardcut_baked;
        vl3d_set_error("unsupported with act_order VL3D_ACT_BAKED: built is (affine, hardcut, baked) with sigmoid / sigmoid activations, fp32 and fp16 stacks");
        return nullptr;
    }
    vl3d_set_error("unsupported (coord_mode, border_mode, act_order): built are (utils_mpi, zeros, pre|post), (utils_mpi, hardcut, pre), "
                   "(affine, hardcut, post), (affine, hardcut, baked)");
    return nullptr;
}
int dispatch(bool bwd, const vl3d_render_desc *d, const RenderArgs &a, hipStream_t s) {
    const ConvFn conv = conv_of(d);
    return conv ? conv(bwd, d, a, s) : VL3D_EUNSUPPORTED;
}

int check_desc(const vl3d_render_desc *d) {
    VL3D_REQUIRE(d != nullptr, "null render desc");
    if (vl3d_check_variant(d->variant) != VL3D_OK) return VL3D_EINVAL;
    VL3D_REQUIRE(d->D > 0 && d->T > 0 && d->Hs > 0 && d->Ws > 0 && d->H > 0 && d->W > 0, "non-positive render dims");
    VL3D_REQUIRE((int64_t)d->Hs * d->Ws < (1ll << 31), "plane too large for 32-bit texel index");
    VL3D_REQUIRE(d->Hs < (1 << 24) && d->Ws < (1 << 24), "plane side too large (24-bit row arithmetic)");
    VL3D_REQUIRE(d->stack_dtype == VL3D_F32 || d->stack_dtype == VL3D_F16, "stack_dtype must be VL3D_F32 or VL3D_F16");
    VL3D_REQUIRE(d->coord_mode != VL3D_COORD_AFFINE_PLANES || (d->sx == 1.0f && d->sy == 1.0f && d->ox == 0.0f && d->oy == 0.0f),
                 "VL3D_COORD_AFFINE_PLANES: the texel transforms live in the per-plane records (sx = sy = 1, ox = oy = 0)");
    VL3D_REQUIRE(d->stack_dtype == VL3D_F32 || (d->rgb_act == VL3D_ACT_SIGMOID && d->alpha_act == VL3D_ACT_SIGMOID),
                 "fp16 plane stacks are implemented for the shipped (sigmoid, sigmoid) activations only");
    // the packed fp16 tap load fetches texels x0 and x0+1 of a row with one 16-byte read (load_taps2): a row needs two texels
    VL3D_REQUIRE(d->stack_dtype == VL3D_F32 || d->Ws >= 2, "fp16 plane stacks need Ws >= 2");
    VL3D_REQUIRE(d->uv_noise_seed == 0 || (d->border_mode == VL3D_BORDER_HARDCUT && d->coord_mode != VL3D_COORD_UTILS_MPI),
                 "uv_noise_seed (add_uv_noise, MPV.py:420-423) belongs to the planar MPV / MPI convention: affine coordinates, VL3D_BORDER_HARDCUT");
    return VL3D_OK;
}

// tile culling of the float render (quad_keep NULL: a dense model, the grid is not read): the shared grid rules (vl3d_render_args.h) plus
// what only this unit's conventions need, `who` in front of the message
int check_cull(const vl3d_render_desc *desc, const uint8_t *quad_keep, int32_t QH, int32_t QW, const char *who) {
    if (!quad_keep) return VL3D_OK;
    if (desc->coord_mode == VL3D_COORD_AFFINE_PLANES) return refuse(who, "tile culling is not available with per-plane texel transforms");
    const int rc = check_cull_grid(desc, QH, QW, who);
    if (rc != VL3D_OK) return rc;
    if (!(QH > 0 || (desc->coord_mode == VL3D_COORD_AFFINE && desc->border_mode == VL3D_BORDER_HARDCUT)))
        return refuse(who, "tile-exact layout: the planar MPV / MPI convention only (VL3D_COORD_AFFINE, VL3D_BORDER_HARDCUT)");
    return VL3D_OK;
}

}  // namespace

extern "C" int64_t vl3d_render_cull_scratch_bytes(const vl3d_render_desc *desc) {
    if (!desc || desc->H <= 0 || desc->W <= 0) return 0;
    // two 64-bit plane masks per forward workgroup, sized for the smallest workgroup any forward variant uses (64 x 4 pixels)
    return (int64_t)((desc->W + 63) / 64) * ((desc->H + 3) / 4) * 16;
}

// scratch layout: per-plane records | one int4 window per (tile, plane), as many as the region shape with the most tiles needs
// (bwd_max_tiles, vl3d_render_bwd_choice.h) | (256-byte aligned) owner table, one uint16 per (plane, texel)
static int64_t owner_table_off(const vl3d_render_desc *desc) {
    const int64_t b = (int64_t)plan_win_off(desc->D) * sizeof(float) + bwd_max_tiles(desc->H, desc->W) * desc->D * 16;
    return (b + 255) & ~(int64_t)255;
}

extern "C" int64_t vl3d_render_bwd_scratch_bytes(const vl3d_render_desc *desc) {
    if (!desc || desc->D <= 0 || desc->H <= 0 || desc->W <= 0) return 0;
    // + padding: the gather's unconditional prefetch reads up to 16 rows + 64 texels past a window's corner
    return owner_table_off(desc) + ((int64_t)desc->D * desc->Hs * desc->Ws + 16 * (int64_t)desc->Ws + 64) * 2;
}

static void set_reg_state(RenderArgs &a, const vl3d_render_desc *d, const void *reg_state);
static int check_mask_desc(const vl3d_render_desc *d, const char *who);
static int check_adam_desc(const vl3d_render_desc *desc, bool has_quad_map);

// ---- what the three backward entries share ----------------------------------------------------------------------------------------------
// the forward's inputs and saved outputs, the incoming gradients and the gradient to write
static void set_bwd_io(RenderArgs &a, const vl3d_render_desc *desc, const void *stack, const float *homos, const float *rgb, const float *alpha,
                       const float *grad_rgb, const float *grad_alpha, const float *grad_reg, const void *reg_state, const float *grad_alpha_sums,
                       float *grad_stack) {
    if (grad_reg) set_reg_state(a, desc, reg_state);
    a.stack = (const float *)stack; a.homos = homos;
    a.rgb = const_cast<float *>(rgb); a.alpha = const_cast<float *>(alpha);
    a.g_rgb = grad_rgb; a.g_alpha = grad_alpha; a.g_reg = grad_reg; a.g_asum = grad_alpha_sums; a.g_stack = grad_stack;
}
// the call's policy; with an owner-computes path: the plan and the owner table inside the caller's scratch
static void set_bwd_setting(RenderArgs &a, const vl3d_render_desc *desc, const BwdSetting &set, void *scratch) {
    a.bwd_policy = set.policy; a.gather9 = set.gather9; a.owner4 = set.owner4;
    if (set.policy == BWD_NONE) return;
    a.plan = (const float *)scratch;
    a.owner = reinterpret_cast<const unsigned short *>(reinterpret_cast<const char *>(scratch) + owner_table_off(desc));
}
// the owner-computes kernels may take the call: enough scratch (0 bytes: none), and no add_uv_noise -- a jittered tap can leave the 1-pixel
// halo they stage
static bool bwd_tile_ok(const vl3d_render_desc *desc, int64_t scratch_bytes) {
    return scratch_bytes >= vl3d_render_bwd_scratch_bytes(desc) && desc->uv_noise_seed == 0;
}

extern "C" int vl3d_render_bwd_choice(const vl3d_render_desc *desc, int32_t entry, int32_t has_quad_keep, int32_t has_reg_grads,
                                      int64_t scratch_bytes, int32_t fused_step, vl3d_bwd_choice *out) {
    int rc = check_desc(desc);
    if (rc != VL3D_OK) return rc;
    VL3D_REQUIRE(out != nullptr, "vl3d_render_bwd_choice: null out");
    VL3D_REQUIRE(entry >= VL3D_BWD_ENTRY_RENDER && entry <= VL3D_BWD_ENTRY_ADAM && (fused_step != 0) == (entry == VL3D_BWD_ENTRY_ADAM),
                 "vl3d_render_bwd_choice: entry is VL3D_BWD_ENTRY_RENDER, _MASK or _ADAM, and fused_step names the last");
    if (entry == VL3D_BWD_ENTRY_MASK) {
        rc = check_mask_desc(desc, "vl3d_render_bwd_mask");
        if (rc != VL3D_OK) return rc;
        VL3D_REQUIRE(!has_quad_keep && desc->uv_noise_seed == 0, "vl3d_render_bwd_mask: dense models without add_uv_noise");
    }
    if (entry == VL3D_BWD_ENTRY_ADAM) {
        rc = check_adam_desc(desc, has_quad_keep != 0);
        if (rc != VL3D_OK) return rc;
        VL3D_REQUIRE(desc->uv_noise_seed == 0 && scratch_bytes >= vl3d_render_bwd_scratch_bytes(desc),
                     "vl3d_render_bwd_adam: no add_uv_noise, scratch of vl3d_render_bwd_scratch_bytes()");
    }
    if (!conv_of(desc)) return VL3D_EUNSUPPORTED;
    VL3D_REQUIRE(!has_quad_keep || desc->coord_mode != VL3D_COORD_AFFINE_PLANES, "tile culling is not available with per-plane texel transforms");
    // the RenderArgs the entry would build, as far as the choice reads them (a flag the entries carry as a pointer: any non-null address, never
    // dereferenced), then the launch's own bwd_facts_of() with the convention the descriptor dispatches to
    static const float present = 0.0f;
    const bool adam = entry == VL3D_BWD_ENTRY_ADAM, qk = has_quad_keep != 0;
    RenderArgs a = render_args_of(desc);
    a.g_reg = has_reg_grads ? &present : nullptr;
    a.mask = entry == VL3D_BWD_ENTRY_MASK ? &present : nullptr;
    a.ad.p = adam ? reinterpret_cast<float4 *>(const_cast<float *>(&present)) : nullptr;
    a.quad_keep = qk ? reinterpret_cast<const unsigned char *>(&present) : nullptr;
    a.g_f16 = desc->stack_dtype == VL3D_F16;
    a.grad_culled_unwritten = (qk && (adam || (desc->grad_flags & VL3D_GRAD_CULLED_UNWRITTEN))) ? 1 : 0;
    const BwdSetting set = bwd_setting_of(entry, desc->variant & 0xf, bwd_tile_ok(desc, scratch_bytes), qk);
    a.bwd_policy = set.policy; a.gather9 = set.gather9; a.owner4 = set.owner4;
    const bool planes = desc->coord_mode == VL3D_COORD_AFFINE_PLANES;      // compiled as VL3D_COORD_AFFINE with 16-float plane records
    const BwdFacts f = bwd_facts_of(a, planes ? VL3D_COORD_AFFINE : desc->coord_mode, desc->border_mode, desc->act_order, desc->rgb_act, desc->alpha_act,
                                    a.g_f16 != 0, planes ? 16 : 9);
    const BwdChoice c = choose_bwd(f);
    const bool none = c.family == VL3D_BWD_ATOMICS;
    *out = vl3d_bwd_choice{c.family, none ? 0 : BWD_REGIONS[c.shape].width, none ? 0 : BWD_REGIONS[c.shape].rows,
                           c.reg, c.mask, c.adam, c.cull, c.f16, c.owner4, f.set.gather9};
    return VL3D_OK;
}

// reg_state: flags [H][W] u8 | coverage masks [H][W][2] u64 | sign words [ceil(D/4)][T][H][W][4] u16 | patch words (same shape) (256-byte aligned parts)
struct RegLayout { int64_t masks, signs, patch, total; };
static RegLayout reg_layout(const vl3d_render_desc *d) {
    auto up = [](int64_t v) { return (v + 255) & ~(int64_t)255; };
    const int64_t px = (int64_t)d->H * d->W, words = (int64_t)((d->D + 3) / 4) * d->T * px * 8;      // groups of four planes
    RegLayout l;
    l.masks = up(px);
    l.signs = l.masks + up(px * 16);
    l.patch = l.signs + up(words);
    l.total = l.patch + up(words);
    return l;
}
static void set_reg_state(RenderArgs &a, const vl3d_render_desc *d, const void *reg_state) {
    char *b = reinterpret_cast<char *>(const_cast<void *>(reg_state));
    const RegLayout l = reg_layout(d);
    a.reg_flags = reinterpret_cast<unsigned char *>(b);
    a.reg_masks = reinterpret_cast<unsigned long long *>(b + l.masks);
    a.reg_signs = reinterpret_cast<unsigned short *>(b + l.signs);
    a.reg_patch = reinterpret_cast<unsigned short *>(b + l.patch);
}
extern "C" int64_t vl3d_render_reg_state_bytes(const vl3d_render_desc *desc) {
    if (!desc || desc->D <= 0 || desc->T <= 0 || desc->H <= 0 || desc->W <= 0) return 0;
    return reg_layout(desc).total;
}

// ---- stage 1's loop mask as a fifth composited channel (MPI.py:115-117, 568-583) ---------------------------------------------------
static int check_mask_desc(const vl3d_render_desc *d, const char *who) {
    if (d->coord_mode == VL3D_COORD_AFFINE && d->border_mode == VL3D_BORDER_HARDCUT && d->act_order == VL3D_ACT_POST &&
        d->rgb_act == VL3D_ACT_SIGMOID && d->alpha_act == VL3D_ACT_SIGMOID && d->stack_dtype == VL3D_F32)
        return VL3D_OK;
    vl3d_set_error((std::string(who) + ": the loop-mask channel is built for the planar convention stage 1 ships -- (affine, hardcut, post), "
                   "sigmoid / sigmoid, fp32 stack (MPI.py:452-594); render the label in a pass of its own otherwise").c_str());
    return VL3D_EUNSUPPORTED;
}

// ---- the five forwards: one body ------------------------------------------------------------------------------------------------------
// An entry passes NULL / 0 for what it does not take.  quad_keep NULL: a dense model -- QH, QW and cull_scratch are not read.
enum FwdEntry { FWD, FWD_FRAMES, FWD_REG, REG_FWD, FWD_MASK };

static int render_fwd(FwdEntry e, const char *who, const vl3d_render_desc *desc, const void *stack, const float *mask, int32_t frame0,
                      int32_t T_alloc, const float *homos, const uint8_t *quad_keep, int32_t QH, int32_t QW, void *cull_scratch, float *rgb,
                      float *alpha, float *label, float *alpha_sums, double *sums, void *reg_state, vl3d_stream_t stream) {
    int rc = check_desc(desc);
    if (rc != VL3D_OK) return rc;
    const bool plain = e == FWD || e == FWD_FRAMES;      // the render alone
    const bool image = e != REG_FWD;                     // rgb / alpha are written
    if (e == FWD_MASK) {
        rc = check_mask_desc(desc, who);
        if (rc != VL3D_OK) return rc;
        if (!(mask && label)) return refuse(who, "null pointer");
        if (desc->uv_noise_seed != 0)
            return refuse(who, "add_uv_noise jitters the colour samples only (MPI.py:519-522, 568-572): render the label in a pass of its own");
        if ((sums == nullptr) != (reg_state == nullptr)) return refuse(who, "sums and reg_state come together (both NULL: no layer regularisers)");
    }
    const bool reg = e == FWD_REG || e == REG_FWD || (e == FWD_MASK && sums);      // the layer regularisers' sums are formed
    if (!(stack && homos && (!image || (rgb && alpha)) && (!reg || (sums && reg_state)))) return refuse(who, "null pointer");
    if (reg && desc->D > 128) return refuse(who, "the layer regularisers support at most 128 planes (coverage masks)");
    if (!quad_keep) { QH = QW = 0; cull_scratch = nullptr; }
    rc = check_cull(desc, quad_keep, QH, QW, who);
    if (rc != VL3D_OK) return rc;
    // (the regulariser kernels walk the quad map themselves: only the render alone plans with plane masks)
    if (plain && quad_keep && !cull_scratch) return refuse(who, "tile culling: the forward needs vl3d_render_cull_scratch_bytes() of scratch");
    if (!((int64_t)desc->Hs * desc->Ws * 16 < (1ll << 32))) return refuse(who, "frame too large for 32-bit byte offsets");
    RenderArgs a = render_args_of(desc);
    a.stack = (const float *)stack; a.homos = homos; a.rgb = rgb; a.alpha = alpha; a.asum = alpha_sums;
    a.mask = mask; a.label = label;
    a.quad_keep = quad_keep;
    set_cull_geometry(a, desc, QH, QW);
    if (plain) a.cull_masks = (const unsigned long long *)cull_scratch;
    if (plain || e == FWD_MASK) a.fwd_variant = (desc->variant >> 8) & 0xf;
    if (plain) a.ablate = (desc->variant >> 4) & 0xf;
    a.g_f16 = desc->stack_dtype == VL3D_F16;      // (the mask forward is fp32 by refusal)
    if (reg) {
        a.reg_sums = sums;      // (cleared by reg_masks_k, the first kernel of the regulariser forward)
        set_reg_state(a, desc, reg_state);
        // 1: the sums alone | 2: render + sums in one sweep | 3: a tile-culled model's slot kernel composites the render as it goes
        a.reg_fwd = e == REG_FWD ? 1 : (quad_keep ? 3 : 2);
    }
    if (e == FWD_FRAMES) {      // frames frame0 .. frame0 + T - 1 of a (D, T_alloc, Hs, Ws, 4) allocation, read in place
        if (T_alloc <= 0) return refuse(who, "T_alloc must be the clip length of the stack allocation");
        if (!(frame0 >= 0 && frame0 + desc->T <= T_alloc)) return refuse(who, "the run of frames leaves the clip");
        a.stack = reinterpret_cast<const float *>(reinterpret_cast<const char *>(stack) + (size_t)frame0 * desc->Hs * desc->Ws * (a.g_f16 ? 8 : 16));
        a.Tstride = T_alloc;
    }
    rc = dispatch(false, desc, a, (hipStream_t)stream);
    if (rc != VL3D_OK) return rc;
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}

extern "C" int vl3d_render_fwd(const vl3d_render_desc *desc, const void *stack, const float *homos, const uint8_t *quad_keep, int32_t QH,
                               int32_t QW, void *cull_scratch, float *rgb, float *alpha, float *alpha_sums, vl3d_stream_t stream) {
    return render_fwd(FWD, "vl3d_render_fwd", desc, stack, nullptr, 0, 0, homos, quad_keep, QH, QW, cull_scratch, rgb, alpha, nullptr, alpha_sums,
                      nullptr, nullptr, stream);
}

extern "C" int vl3d_render_fwd_frames(const vl3d_render_desc *desc, const void *stack, int32_t frame0, int32_t T_alloc, const float *homos,
                                      const uint8_t *quad_keep, int32_t QH, int32_t QW, void *cull_scratch, float *rgb, float *alpha,
                                      vl3d_stream_t stream) {
    return render_fwd(FWD_FRAMES, "vl3d_render_fwd_frames", desc, stack, nullptr, frame0, T_alloc, homos, quad_keep, QH, QW, cull_scratch, rgb,
                      alpha, nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int vl3d_render_fwd_reg(const vl3d_render_desc *desc, const void *stack, const float *homos, const uint8_t *quad_keep, int32_t QH,
                                   int32_t QW, float *rgb, float *alpha, float *alpha_sums, double *sums, void *reg_state,
                                   vl3d_stream_t stream) {
    return render_fwd(FWD_REG, "vl3d_render_fwd_reg", desc, stack, nullptr, 0, 0, homos, quad_keep, QH, QW, nullptr, rgb, alpha, nullptr,
                      alpha_sums, sums, reg_state, stream);
}

extern "C" int vl3d_render_reg_fwd(const vl3d_render_desc *desc, const void *stack, const float *homos, const uint8_t *quad_keep, int32_t QH,
                                   int32_t QW, double *sums, void *reg_state, vl3d_stream_t stream) {
    return render_fwd(REG_FWD, "vl3d_render_reg_fwd", desc, stack, nullptr, 0, 0, homos, quad_keep, QH, QW, nullptr, nullptr, nullptr, nullptr,
                      nullptr, sums, reg_state, stream);
}

extern "C" int vl3d_render_fwd_mask(const vl3d_render_desc *desc, const void *stack, const float *mask, const float *homos, float *rgb,
                                    float *alpha, float *label, float *alpha_sums, double *sums, void *reg_state, vl3d_stream_t stream) {
    return render_fwd(FWD_MASK, "vl3d_render_fwd_mask", desc, stack, mask, 0, 0, homos, nullptr, 0, 0, nullptr, rgb, alpha, label, alpha_sums,
                      sums, reg_state, stream);
}

extern "C" int vl3d_render_bwd_mask(const vl3d_render_desc *desc, const void *stack, const float *mask, const float *homos, const float *rgb,
                                    const float *alpha, const float *grad_rgb, const float *grad_alpha, const float *grad_label,
                                    const float *grad_reg, const void *reg_state, const float *grad_alpha_sums, float *grad_stack,
                                    float *grad_mask, void *scratch, int64_t scratch_bytes, vl3d_stream_t stream) {
    int rc = check_desc(desc);
    if (rc != VL3D_OK) return rc;
    rc = check_mask_desc(desc, "vl3d_render_bwd_mask");
    if (rc != VL3D_OK) return rc;
    VL3D_REQUIRE(stack && mask && homos && rgb && alpha && grad_rgb && grad_label && grad_stack && grad_mask, "null pointer passed to vl3d_render_bwd_mask");
    VL3D_REQUIRE(!grad_reg || reg_state, "vl3d_render_bwd_mask: grad_reg needs the reg_state the forward with regularisers filled");
    VL3D_REQUIRE((int64_t)desc->Hs * desc->Ws * 16 < (1ll << 32), "frame too large for 32-bit byte offsets");
    RenderArgs a = render_args_of(desc);
    set_bwd_io(a, desc, stack, homos, rgb, alpha, grad_rgb, grad_alpha, grad_reg, reg_state, grad_alpha_sums, grad_stack);
    a.mask = mask; a.g_label = grad_label; a.g_mask = grad_mask;
    VL3D_REQUIRE(desc->uv_noise_seed == 0, "vl3d_render_bwd_mask: add_uv_noise jitters the colour samples only (MPI.py:519-522, 568-572): render the label in a pass of its own");
    const BwdSetting set = bwd_setting_of(VL3D_BWD_ENTRY_MASK, desc->variant & 0xf, bwd_tile_ok(desc, scratch ? scratch_bytes : 0), false);
    set_bwd_setting(a, desc, set, scratch);
    if (set.policy == BWD_NONE) {
        const size_t texels = (size_t)desc->D * desc->T * desc->Hs * desc->Ws;
        VL3D_HIP(hipMemsetAsync(grad_stack, 0, texels * 16, (hipStream_t)stream));
        VL3D_HIP(hipMemsetAsync(grad_mask, 0, texels * 4, (hipStream_t)stream));
    }
    rc = dispatch(true, desc, a, (hipStream_t)stream);
    if (rc != VL3D_OK) return rc;
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}

// quad_keep NULL: a dense model -- QH and QW are not read
extern "C" int vl3d_render_bwd(const vl3d_render_desc *desc, const void *stack, const float *homos, const uint8_t *quad_keep, int32_t QH,
                               int32_t QW, const float *rgb, const float *alpha, const float *grad_rgb, const float *grad_alpha,
                               const float *grad_reg, const void *reg_state, const float *grad_alpha_sums, float *grad_stack, void *scratch,
                               int64_t scratch_bytes, vl3d_stream_t stream) {
    int rc = check_desc(desc);
    if (rc != VL3D_OK) return rc;
    if (!quad_keep) QH = QW = 0;
    rc = check_cull(desc, quad_keep, QH, QW, "vl3d_render_bwd");
    if (rc != VL3D_OK) return rc;
    VL3D_REQUIRE(stack && homos && rgb && alpha && grad_rgb && grad_stack, "vl3d_render_bwd: null pointer");
    VL3D_REQUIRE(!grad_reg || reg_state, "vl3d_render_bwd: grad_reg needs the reg_state the forward with regularisers filled");
    RenderArgs a = render_args_of(desc);
    set_bwd_io(a, desc, stack, homos, rgb, alpha, grad_rgb, grad_alpha, grad_reg, reg_state, grad_alpha_sums, grad_stack);
    a.quad_keep = quad_keep;
    set_cull_geometry(a, desc, QH, QW);
    a.g_f16 = desc->stack_dtype == VL3D_F16;
    a.grad_culled_unwritten = (quad_keep && (desc->grad_flags & VL3D_GRAD_CULLED_UNWRITTEN)) ? 1 : 0;
    a.ablate = (desc->variant >> 4) & 0xf;
    const BwdSetting set = bwd_setting_of(VL3D_BWD_ENTRY_RENDER, desc->variant & 0xf, bwd_tile_ok(desc, scratch ? scratch_bytes : 0), quad_keep != nullptr);
    set_bwd_setting(a, desc, set, scratch);
    if (set.policy == BWD_NONE) {
        const size_t bytes = (size_t)desc->D * desc->T * desc->Hs * desc->Ws * (desc->stack_dtype == VL3D_F16 ? 8 : 16);
        VL3D_HIP(hipMemsetAsync(grad_stack, 0, bytes, (hipStream_t)stream));
    }
    rc = dispatch(true, desc, a, (hipStream_t)stream);
    if (rc != VL3D_OK) return rc;
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}

// ---- the optimiser step inside the backward (include/vl3d.h) ---------------------------------------------------------------------------
extern "C" int64_t vl3d_render_bwd_adam_class_bytes(const vl3d_render_desc *desc) {
    if (!desc || desc->D <= 0 || desc->Hs <= 0 || desc->Ws <= 0) return 0;
    // one 8-byte record per (plane, texel) of the compact window, padded like the owner table (the gather's unconditional prefetch)
    return ((int64_t)desc->D * desc->Hs * desc->Ws + 16 * (int64_t)desc->Ws + 64) * 8;
}

static int check_adam_desc(const vl3d_render_desc *desc, bool has_quad_map) {
    const int bv = desc->variant & 0xf;
    if (!(desc->coord_mode == VL3D_COORD_AFFINE && desc->border_mode == VL3D_BORDER_HARDCUT && desc->act_order == VL3D_ACT_POST &&
          desc->rgb_act == VL3D_ACT_SIGMOID && desc->alpha_act == VL3D_ACT_SIGMOID && desc->stack_dtype == VL3D_F32 &&
          (has_quad_map ? (bv == 0 || bv == 3 || bv == 5) : (desc->T >= 2 && bv == 0)))) {
        vl3d_set_error("vl3d_render_bwd_adam: built for the stage-2 iteration -- (affine, hardcut, post), sigmoid / sigmoid, fp32 stack, "
                       "T >= 2 and variant 0 for a dense model; use vl3d_render_bwd + vl3d_adam_window_step otherwise");
        return VL3D_EUNSUPPORTED;
    }
    return VL3D_OK;
}

// what the owner's fused store needs of a (checked) adam window: its state, geometry and the scalars of its step
static vl3d_adam_epilogue adam_epilogue_of(const vl3d_adam_window &w) {
    const int ts = vl3d_adam::TS;
    const float2 sc = vl3d_adam::adam_step_scalars(w.lr, w.beta1, w.beta2, w.step);
    vl3d_adam_epilogue e{};
    e.p = reinterpret_cast<float4 *>(w.param); e.m = reinterpret_cast<float4 *>(w.exp_avg); e.v = reinterpret_cast<float4 *>(w.exp_avg_sq);
    e.last_step = w.last_step;
    e.boxes = (w.plane_boxes && w.D <= 128) ? reinterpret_cast<const int4 *>(w.boxes_scratch) : nullptr;
    e.y0 = w.y0; e.x0 = w.x0; e.Hs = w.Hs; e.Ws = w.Ws;
    e.tiles_y = (w.Hs + ts - 1) / ts; e.tiles_x = (w.Ws + ts - 1) / ts;
    e.step = (int)w.step;
    e.lr_bc1 = sc.x; e.beta1 = w.beta1; e.beta2 = w.beta2; e.eps = w.eps; e.bc2s = sc.y;
    e.quad_dyn = w.quad_keep ? w.quad_dyn : nullptr;
    e.cls = w.quad_keep ? reinterpret_cast<uint2 *>(w.class_scratch) : nullptr;
    e.blocks = w.blocks;
    return e;
}

extern "C" int vl3d_render_bwd_adam(const vl3d_render_desc *desc, const void *stack, const float *homos, const float *rgb, const float *alpha,
                                    const float *grad_rgb, const float *grad_alpha, const float *grad_reg, const void *reg_state,
                                    const float *grad_alpha_sums, float *grad_stack, void *scratch, int64_t scratch_bytes,
                                    const vl3d_adam_window *adam, vl3d_stream_t stream) {
    int rc = check_desc(desc);
    if (rc != VL3D_OK) return rc;
    VL3D_REQUIRE(adam != nullptr, "vl3d_render_bwd_adam: null adam window");
    if (desc->uv_noise_seed) {
        vl3d_set_error("vl3d_render_bwd_adam: add_uv_noise takes the atomics backward (vl3d_render_bwd + vl3d_adam_window_step)");
        return VL3D_EUNSUPPORTED;
    }
    VL3D_REQUIRE(stack && homos && rgb && alpha && grad_rgb && grad_stack && scratch, "null pointer passed to vl3d_render_bwd_adam");
    VL3D_REQUIRE(!grad_reg || reg_state, "vl3d_render_bwd_adam: grad_reg needs the reg_state the forward with regularisers filled");
    const uint8_t *qk = adam->quad_keep;
    rc = check_adam_desc(desc, qk != nullptr);
    if (rc != VL3D_OK) return rc;
    VL3D_REQUIRE(scratch_bytes >= vl3d_render_bwd_scratch_bytes(desc), "vl3d_render_bwd_adam: scratch smaller than vl3d_render_bwd_scratch_bytes()");
    VL3D_REQUIRE(adam->param && adam->exp_avg && adam->exp_avg_sq && adam->last_step && adam->hist && adam->step >= 1 &&
                     adam->step < (1ll << 31), "vl3d_render_bwd_adam: null pointer / bad step in the adam window");
    VL3D_REQUIRE((int64_t)desc->Hs * desc->Ws * 16 < (1ll << 32) && (int64_t)adam->Hs * adam->Ws * 16 < (1ll << 32),
                 "frame too large for 32-bit byte offsets");
    if (qk) {
        rc = check_cull(desc, qk, adam->QH, adam->QW, "vl3d_render_bwd_adam");
        if (rc != VL3D_OK) return rc;
        VL3D_REQUIRE(adam->class_scratch, "vl3d_render_bwd_adam: a tile-culled model needs class_scratch (vl3d_render_bwd_adam_class_bytes())");
        VL3D_REQUIRE(adam->step < (1ll << 29), "vl3d_render_bwd_adam: tile-culled models keep the step in 29 bits of the texel records");
    } else {
        VL3D_REQUIRE(!adam->blocks, "vl3d_render_bwd_adam: the packed layout belongs to a tile-culled model (quad maps)");
    }
    if (qk) {
        VL3D_REQUIRE(desc->cull_Hs == adam->Hs && desc->cull_Ws == adam->Ws && desc->cull_row0 == adam->y0 && desc->cull_col0 == adam->x0,
                     "vl3d_render_bwd_adam: desc->cull_* must name the optimiser's window (y0, x0) of its (Hs, Ws) planes");
    }
    VL3D_REQUIRE(adam->D == desc->D && adam->T == desc->T && adam->wh == desc->Hs && adam->ww == desc->Ws,
                 "vl3d_render_bwd_adam: the adam window's D, T, wh, ww must be desc->D, desc->T, desc->Hs, desc->Ws (the stack is the window's compact copy)");
    hipStream_t s = (hipStream_t)stream;
    rc = vl3d_adam_window_before_render(*adam, s);
    if (rc != VL3D_OK) return rc;
    RenderArgs a = render_args_of(desc);
    set_bwd_io(a, desc, stack, homos, rgb, alpha, grad_rgb, grad_alpha, grad_reg, reg_state, grad_alpha_sums, grad_stack);
    a.quad_keep = qk; a.QH = adam->QH; a.QW = adam->QW;
    set_cull_geometry(a, desc, adam->QH, adam->QW);
    a.grad_culled_unwritten = qk ? 1 : 0;
    set_bwd_setting(a, desc, bwd_setting_of(VL3D_BWD_ENTRY_ADAM, desc->variant & 0xf, true, qk != nullptr), scratch);
    a.ad = adam_epilogue_of(*adam);
    rc = dispatch(true, desc, a, s);
    if (rc != VL3D_OK) return rc;
    // behind the backward, under the plan's device-side flag: nothing more (dense, feasible) / the static texels (tile-culled, feasible) / the
    // whole window from the atomics kernel's gradient (infeasible view); the tiles are marked either way
    return vl3d_adam_window_behind_render(*adam, grad_stack, reinterpret_cast<const int *>(scratch), s);
}
