/* vl3d.h -- C ABI of the MI355X-native MPI/MPV render-and-composite + looping-loss hot path.
 *
 * One shared library (videoloop3d_amd/lib/libvl3d_hip.so, built by hipcc for gfx950) exports
 * exactly these symbols.  Plain pointers and sizes only: no torch types.  The reference
 * (limacv/VideoLoop3D) is pure Python and has no FFI; each entry point cites the reference
 * operator (file:line in /root/reference) it replaces, and INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add.
 *
 * Contract:
 *   - every pointer is a DEVICE pointer owned by the caller; the library never allocates or frees
 *     and never synchronises; all work is enqueued on `stream` (a hipStream_t passed as void*).
 *   - all tensors are dense row-major fp32 unless stated; outputs are overwritten (the library
 *     zero-fills accumulation targets itself on the same stream).
 *   - return value: VL3D_OK or an error code; never aborts.  vl3d_last_error() gives a message.
 */
#ifndef VL3D_H
#define VL3D_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *vl3d_stream_t; /* hipStream_t */

enum { VL3D_OK = 0, VL3D_EINVAL = 1, VL3D_ELAUNCH = 2, VL3D_EUNSUPPORTED = 3 };

/* activation table: MPI.py:21-31 (ACTIVATES); shipped configs use sigmoid for rgb and alpha
 * (configs/mpv_base.txt:29-30). */
enum { VL3D_ACT_NONE = 0, VL3D_ACT_SIGMOID = 1, VL3D_ACT_RELU = 2, VL3D_ACT_CLAMP = 3, VL3D_ACT_ABS = 4 };
/* texel-coordinate convention.  UTILS_MPI: g = p/[Ws/2,Hs/2]-1 then grid_sample(align_corners=True),
 * i.e. texel = p*(size-1)/size (utils_mpi.py:173-175).  AFFINE: texel = p*s + o (MPV.py atlas-cell UV). */
enum { VL3D_COORD_UTILS_MPI = 0, VL3D_COORD_AFFINE = 1, VL3D_COORD_AFFINE_PLANES = 2 };
/* AFFINE_PLANES (with BORDER_HARDCUT, ACT_POST, sigmoid/sigmoid): every plane has its OWN affine texel transform and quad extent --
 * the reference's atlas-cell layout, where plane p of an atlas of grid_h x grid_w cells samples at xm*pitch - (p % grid_w)/grid_w
 * with pitch = (Aw-1)/(grid_w*(mpi_w-1)) and is covered while 0 <= xm <= mpi_w-1 (MPV.py:75-81, 394-439).  `homos` is then
 * (D,16): per plane the 3x3 matrix target pixel -> TEXEL coordinate (the plane's transform already folded in), then the coverage
 * box x0, x1, y0, y1 in texel coordinates (inclusive), 3 floats of padding; desc->sx = sy = 1, ox = oy = 0. */
/* ZEROS: grid_sample padding_mode='zeros' (utils_mpi.py:174).  HARDCUT: quad extent, uncovered -> 0 after
 * activation (MPV.py:389,441-447). */
enum { VL3D_BORDER_ZEROS = 0, VL3D_BORDER_HARDCUT = 1 };
/* PRE: activate texels, then sample (sigmoid -> warp_homography chain).  POST: sample, then activate (MPV.py:425-435).
 * BAKED: the render of the model the viewer package shows ("Baked playback" below), differentiable -- training under the bake rule.
 * Per tap and channel, with s the stored logit:
 *     a = act(s);  u = uint8(trunc(clip(a * 255, 0, 255)))  (THE bake rule: the byte vl3d_bake_rgba8 writes for that texel, bit for bit --
 *     one device function serves both);  v = (float)u / 255  (the decoded texel; the 1 / 255 is folded into the four tent weights);
 *     the four v are blended with the tent weights, then coverage and composite exactly as PRE.
 *     backward: dL/ds = dL/dv * act'(s) with act'(s) from the UNROUNDED a -- PRE's gradient, the rounding is straight-through.
 * Built for the planar MPV convention (VL3D_COORD_AFFINE, VL3D_BORDER_HARDCUT), sigmoid / sigmoid, fp32 and fp16 stacks: vl3d_render_fwd,
 * _fwd_frames, _fwd_reg, _reg_fwd and vl3d_render_bwd, dense and tile-culled (shared-border and tile-exact).  Every other geometry or
 * activation pair with it is VL3D_EUNSUPPORTED; the loop-mask channel, vl3d_render_fwd_packed, the plane-rows band and
 * vl3d_render_bwd_adam keep refusing everything but POST. */
enum { VL3D_ACT_PRE = 0, VL3D_ACT_POST = 1, VL3D_ACT_BAKED = 2 };
enum { VL3D_F32 = 0, VL3D_F16 = 1, VL3D_U8 = 2 };
/* VL3D_U8: the baked RGBA8 texels of the playback model (vl3d_bake_rgba8 / vl3d_render_fwd_baked below) -- accepted by
 * vl3d_render_fwd_baked and vl3d_render_fwd_baked_pool alone; every other entry point returns VL3D_EINVAL for it. */

const char *vl3d_last_error(void);
/* Raised by one whenever an exported signature or the layout of a struct of this header changes (101: the vl3d_adam_window family takes the
 * struct; 102: vl3d_render_sh_fwd / _bwd); a caller built against another header compares it before its first call. */
int vl3d_version(void);

/* ------------------------------------------------------------------------------------------------
 * Fused render: per-plane homography warp + bilinear sample + activation + front-to-back over
 * composite across D planes.  Replaces the chain MPV.py:351-454 (planar geometry) ==
 * utils_mpi.py:159-176 (warp_homography) + utils_mpi.py:92-107 (overcompose).
 *
 *   stack  : (D, T, Hs, Ws, 4) pre-activation rgba, plane 0 = nearest (MPV.py:51)
 *   homos  : (D, 3, 3) fp32, target pixel -> plane pixel (utils_mpi.py:240-273), shared by all T frames
 *   rgb    : (T, H, W, 3)        alpha : (T, H, W)  = sum of blend weights (MPV.py:454)
 *   row0/col0 : offset of this output window inside the full frame (row-band sharding);
 *               pixel (y,x) of the window is frame pixel (row0+y, col0+x).
 */
typedef struct vl3d_render_desc {
    int32_t D, T, Hs, Ws;
    int32_t H, W;
    int32_t row0, col0;
    int32_t coord_mode, border_mode, act_order, rgb_act, alpha_act;
    int32_t stack_dtype;   /* VL3D_F32 | VL3D_F16 (grad_stack has the same dtype); VL3D_U8: vl3d_render_fwd_baked(_pool) only */
    float pixel_center;    /* 0 (utils_mpi) or 0.5 (pytorch3d pixel centres) */
    float sx, sy, ox, oy;  /* VL3D_COORD_AFFINE only */
    int32_t variant;       /* kernel selector for bitwise cross-checks between EXACT kernels; 0 = default.  Bits 0-3: backward (see
                            * vl3d_render_bwd); bits 8-11: forward -- 6 = one frame and one pixel per thread, 7 = two frames per thread (default for the
                            * shipped activations and T >= 2: a dense fp32 stack two pixel rows per thread, which share their middle tap
                            * row; an fp16 or tile-culled one two frames per thread.  Same bits all three); bits 12-15: 1 = the two-pass forward with regularisers.  Bits 4-7
                            * (timing-only ablations, wrong results) exist only in a -DVL3D_VARIANTS measurement build: the product
                            * library returns VL3D_EINVAL for them. */
    /* tile culling on a WINDOW of the stack (a call with a quad map only; all 0 = the stack is the whole plane): the stack passed in is
     * the texel window [cull_row0, cull_row0+Hs) x [cull_col0, cull_col0+Ws) of a cull_Hs x cull_Ws plane, and the quad grid of
     * quad_keep lies over that whole plane. */
    int32_t cull_row0, cull_col0, cull_Hs, cull_Ws;
    /* vl3d_render_bwd with a quad map only.  Bit 0 (VL3D_GRAD_CULLED_UNWRITTEN): the caller never reads the gradient of texels no kept quad can
     * read (vl3d_adam_window_step / vl3d_adam_step_tiles skip them: they are no parameters), so the texels a workgroup owns on a plane it
     * skips are not written at all instead of being zero-filled -- on a 16 %-kept model that fill was a quarter of the backward's time.
     * Those slots of grad_stack are then UNDEFINED.  0 = every texel of grad_stack is written (a gradient any consumer may read).
     * A permission, not a promise: instantiations without the layer regularisers still write the zeros. */
    int32_t grad_flags;
    /* add_uv_noise of the reference (MPV.py:420-423, MPI.py:519-522; config_parser.py:48; off in every shipped configuration): while training,
     * every sample's UV is jittered by hpix * (2 rand - 1), hpix = 1 / (atlas size - 1) in normalised coordinates = HALF A TEXEL, one draw
     * per (pixel, layer), shared by all frames.  0 = off.  Non-zero: the seed of this call's jitter field -- (jx, jy) uniform in
     * [-0.5, 0.5) texels from a counter hash of (seed, plane, frame pixel): a pure function, so forward, backward and any tiling see the
     * same field (the oracle restates it: oracle/mpi_oracle.uv_jitter_field).  Coverage (hard cut, quad culling) is decided at the UNJITTERED
     * position, as the rasteriser decides it in the reference; the taps move.  VL3D_COORD_AFFINE(_PLANES) with VL3D_BORDER_HARDCUT only; the backward takes the atomics
     * kernel (a jittered tap can leave the owner-computes kernels' 1-pixel halo); vl3d_render_bwd_adam / _fwd_packed refuse it. */
    uint32_t uv_noise_seed;
} vl3d_render_desc;
enum { VL3D_GRAD_CULLED_UNWRITTEN = 1 };

/* alpha_sums (optional, may be NULL): (T,H,W,2) per pixel (sum_k a_k, sum_k a_k^2) over the planes -- the two sums the
 * sparsity regulariser (MPV.py:511-515 / MPI.py:599-603: |a|_1 / |a|_2 per pixel) is made of.
 * quad_keep NULL = a dense model (QH, QW and cull_scratch are not read), else the quad map [D][|QH|][|QW|] of a tile-culled (sparsified)
 * model, its quad grid (negative: tile-exact layout) and vl3d_render_cull_scratch_bytes(desc) bytes of scratch: "Tile culling" below. */
int vl3d_render_fwd(const vl3d_render_desc *desc, const void *stack, const float *homos, const uint8_t *quad_keep, int32_t QH, int32_t QW,
                    void *cull_scratch, float *rgb, float *alpha, float *alpha_sums, vl3d_stream_t stream);
/* ... of frames frame0 .. frame0 + desc->T - 1 of a LONGER clip, read in place: `stack` is the base of a (D, T_alloc, Hs, Ws, 4) allocation,
 * desc->T the number of consecutive frames to render (an evaluation render of single frames or runs of frames -- scripts/script_render_video.py:
 * 129-139 renders one frame per camera of its path -- without gathering `stack[:, ts]` first: 571 MB per 720p frame at D = 32 on 1.1x planes).
 * quad_keep NULL = a dense model, else a tile-culled (sparsified) dense model: vl3d_render_fwd's quad map, grid and scratch, the same run of
 * frames. */
int vl3d_render_fwd_frames(const vl3d_render_desc *desc, const void *stack, int32_t frame0, int32_t T_alloc, const float *homos,
                           const uint8_t *quad_keep, int32_t QH, int32_t QW, void *cull_scratch, float *rgb, float *alpha,
                           vl3d_stream_t stream);

/* Baked playback (csrc/vl3d_render_baked.hip, csrc/vl3d_render_baked_pool.hip).  The viewer package the reference exports
 * (scripts/script_export_mesh.py:117-191) holds ACTIVATED 8-bit atlases, and a player filters those texels bilinearly after the activation --
 * not the picture the float kernels above compute (fp32 texels, interpolate, then activate).
 *   vl3d_bake_rgba8: the one bake rule, per channel u8 = uint8(trunc(clip(act(s) * 255, 0, 255))) -- act = rgb_act (VL3D_ACT_*) for channels
 *     0-2, alpha_act for channel 3; truncation, not rounding (script_export_mesh.py:130-138); straight RGBA, not premultiplied.  stack:
 *     n_texels rgba texels, fp32 (VL3D_F32) or fp16 (VL3D_F16), 16-byte aligned; out: n_texels * 4 bytes.
 *   The render, vl3d_render_fwd_baked / vl3d_render_fwd_baked_pool: desc->T output frames.  Per covered (pixel, plane) the value is the
 *     bilinear blend of the four decoded taps u8 / 255 with NO activation behind it, composited front to back.  Sample
 *     position, hard cut, kept-quad test, tile-exact quad offset and tap weights are the float forward's own device functions: the two
 *     renders agree on every pixel's coverage.  desc: the planar convention only -- VL3D_COORD_AFFINE, VL3D_BORDER_HARDCUT, pixel_center,
 *     sx / sy / ox / oy, stack_dtype = VL3D_U8, uv_noise_seed = 0, variant = 0, Hs, Ws >= 2 (act_order / rgb_act / alpha_act are not read:
 *     the texels are activated already).  Anything else, a NULL pointer, a misaligned source: VL3D_EINVAL, nothing launched.  Forward only;
 *     no host synchronisation.  The two entries differ in the SOURCE; both take the SELECTION and the SINK as the two structs below.
 *   Source.  vl3d_render_fwd_baked: a baked clip (D, T_alloc, Hs, Ws, 4) uint8, 4-byte aligned, read in place.  quad_keep NULL = a dense
 *     model, else vl3d_render_fwd_frames's map, quad grid (negative: tile-exact layout), desc->cull_* window and cull_scratch.
 *     vl3d_render_fwd_baked_pool: the baked POOL of a packed tile-culled model -- the "Packed storage" block table below with RGBA8 texels
 *     behind it.  blocks [D][ceil(Hs/8)][ceil(Ws/8)] int32: -1 (not stored) | slot << 1 | dynamic; pool: n_slots * 256 bytes, a slot = one
 *     8 x 8 block of 4-byte texels, row-major; a static block owns one slot, a dynamic block T_model consecutive ones (frame t at slot + t);
 *     both 4-byte aligned.  A tap in a block without storage reads `culled_rgba8` (r | g << 8 | b << 16 | a << 24).  No desc->cull_* window
 *     (the pool holds whole planes); quad_keep [D][|QH|][|QW|] and cull_scratch are REQUIRED (the table is built from the map), D <= 128.
 *     The table is trusted as packed.PackedLayout builds it: every stored slot (+ T_model - 1 for a dynamic block) lies inside the pool.  Per
 *     covered (pixel, plane): one table entry and one 8-byte load per texel row (two entries and two 4-byte loads where x0 % 8 == 7); static
 *     blocks are fetched once per frame pair; uncovered pixels fetch nothing.  The output has the bits of vl3d_render_fwd_baked on the
 *     unpacked texels.
 *   Selection (vl3d_baked_frames).  A RUN: frames frame0 .. frame0 + desc->T - 1 of the clip's T_alloc (the model's T_model) frames seen by
 *     one camera, homos (D, 3, 3); frame_cam = frame_t = NULL, n_cams = 0; cull_scratch: vl3d_render_cull_scratch_bytes(desc).  A camera
 *     PATH: output frame i is camera frame_cam[i] of homos (n_cams, D, 3, 3), 1 <= n_cams <= 65535, showing frame frame_t[i] -- the spiral of
 *     scripts/script_render_video.py:47-85 -- in ONE plan launch plus ONE render launch; frame0 is not read; cull_scratch:
 *     vl3d_render_path_cull_scratch_bytes(desc, n_cams), two 64-bit plane masks per (camera, 64 x 8 pixel workgroup).  Frame i of a path holds
 *     the bits of the run of frame frame_t[i] alone under camera frame_cam[i].  The host side cannot read the indices: the wrapper
 *     (render.render_path_baked / _pool) range-checks them before it uploads them, and the kernels check them again -- a workgroup whose
 *     camera or frame is out of range returns before any load or store and its pixels stay unwritten.  VL3D_EINVAL: a struct that is neither
 *     (one index pointer NULL, or n_cams != 0 without pointers), a run that leaves the clip, T_alloc / T_model < 1, n_cams outside
 *     [1, 65535], ceil(W/64) * ceil(H/8) * desc->T > 2^31 - 1.
 *   Sink (vl3d_baked_out), exactly one of two.  FLOAT: rgb (N,H,W,3) and alpha (N,H,W) fp32, N = desc->T, as vl3d_render_fwd_frames lays
 *     them out; frames = bg = NULL.  DISPLAY: frames (N, H, W, channels) uint8, channels = 3 (RGB8) or 4 (RGBA8, 4-byte aligned), the frame a
 *     viewer shows, written by the render launch itself (csrc/vl3d_baked_core.h: DisplayOut); rgb = alpha = NULL.  Per pixel, every
 *     operation rounded on its own (the order of the torch statement it replaces; c, A: the float sink's rgb and alpha):
 *         bg != NULL:  x_k = c_k * A + bg[k] * ((-A) + 1)      (MPV.py:455-461)          bg == NULL:  x_k = c_k
 *         byte k = (uint8) trunc(255 * min(max(x_k, 0), 1))    (utils.py to8b);   byte 3 (channels == 4) = trunc(255 * min(max(A, 0), 1)),
 *                                                               never composited over the background
 *     bg: a HOST pointer to 3 finite floats, read by the call (it travels in the kernel arguments).  RGB8 rows are stored lane-packed (a
 *     wave's 192 bytes as 48 dwords) where the 64-pixel row segment is full and 4-byte aligned, as bytes elsewhere; the environment variable
 *     VL3D_DISPLAY_STORE3=bytes selects byte stores everywhere -- a measurement hook (profiles/baked_fwd.py --legs display), same bytes.
 *     VL3D_EINVAL: both sinks or neither, a bg with the float sink, channels outside {3, 4}, misaligned RGBA8 frames, a non-finite bg.
 *   Fractional loop time (vl3d_baked_times; vl3d_render_fwd_baked_times / vl3d_render_fwd_baked_pool_times).  The product is a LOOP of T
 *     frames (T = T_alloc of a clip, T_model of a pool); the baked model at loop time tau in [0, T) is the linear interpolation of its TEXELS
 *     between two adjacent frames, the last and the first included:
 *         t0 = floor(tau),   t1 = t0 + 1 < T ? t0 + 1 : 0 (wraps at the seam),   f = tau - t0
 *     Sample position, coverage, hard cut, kept-quad test, tile-exact offset and tent weights are those of the frame renders above.  Per
 *     covered (pixel, plane), nothing contracted (blend, w255: csrc/vl3d_baked_core.h):
 *         b0_K = blend<K>(taps of frame t0, w255),   b1_K = blend<K>(taps of frame t1, w255),   c_K = fmaf(f, b1_K - b0_K, b0_K),   K = 0..3
 *     (alpha included), and c enters the one-frame composite step unchanged.  Exact consequences: f == 0 gives an output frame the bits of
 *     the path frame (cam, t0); equal taps in both frames (a static block of the pool -- fetched once --, a static quad of a clip, T = 1) give
 *     c_K = b0_K bit for bit at any f.  A path like the one above: output frame i is camera frame_cam[i] of homos (n_cams, D, 3, 3) at time
 *     frame_time[i], one plan launch plus one render launch, one output frame and two source frames per thread; cull_scratch:
 *     vl3d_render_path_cull_scratch_bytes(desc, n_cams); the sink is vl3d_baked_out, float or display.  In the kernel tau is an fp32 value read
 *     from device memory: t0 = (int)tau, f = tau - (float)t0 (exact in fp32); a workgroup whose camera is outside [0, n_cams) or whose tau is
 *     not in [0, T) -- a NaN fails the comparison -- returns before any other load or store and leaves its pixels unwritten.  The wrappers
 *     (render.render_times_baked / _pool) check the times before they upload them; baked.loop_times reduces any real time into [0, T).
 *     A clip: frame t1 at its own offset.  A pool: a static or unstored entry serves both frames from one fetch (or the register), a dynamic
 *     entry is fetched at slot + t0 and slot + t1.  VL3D_EINVAL, nothing launched: what the path form refuses, with its messages, and a NULL
 *     sel, frame_cam or frame_time, reserved != 0, n_cams outside [1, 65535]. */
typedef struct vl3d_baked_frames {
    int32_t frame0;                        /* a run: its first frame */
    int32_t n_cams;                        /* a path: the cameras of homos; 0 for a run */
    const int32_t *frame_cam, *frame_t;    /* a path: device int32[desc->T]; both NULL for a run */
} vl3d_baked_frames;
typedef struct vl3d_baked_out {
    float *rgb, *alpha;                    /* the float sink */
    uint8_t *frames;                       /* the display sink ... */
    int32_t channels;
    const float *bg;                       /* ... its background: host float[3] or NULL */
} vl3d_baked_out;
typedef struct vl3d_baked_times {
    int32_t n_cams;                        /* cameras of homos (n_cams, D, 3, 3), 1 .. 65535 */
    int32_t reserved;                      /* 0 */
    const int32_t *frame_cam;              /* device int32[desc->T] */
    const float *frame_time;               /* device float[desc->T], each in [0, T_alloc) / [0, T_model) */
} vl3d_baked_times;                        /* 24 bytes */
int vl3d_bake_rgba8(int64_t n_texels, const void *stack, int32_t stack_dtype, int32_t rgb_act, int32_t alpha_act, uint8_t *out,
                    vl3d_stream_t stream);
int64_t vl3d_render_path_cull_scratch_bytes(const vl3d_render_desc *desc, int32_t n_cams);
int vl3d_render_fwd_baked(const vl3d_render_desc *desc, const uint8_t *baked, int32_t T_alloc, const float *homos,
                          const vl3d_baked_frames *sel, const uint8_t *quad_keep, int32_t QH, int32_t QW, void *cull_scratch,
                          const vl3d_baked_out *out, vl3d_stream_t stream);
int vl3d_render_fwd_baked_pool(const vl3d_render_desc *desc, const int32_t *blocks, const uint8_t *pool, int32_t T_model, const float *homos,
                               const vl3d_baked_frames *sel, const uint8_t *quad_keep, int32_t QH, int32_t QW, uint32_t culled_rgba8,
                               void *cull_scratch, const vl3d_baked_out *out, vl3d_stream_t stream);
int vl3d_render_fwd_baked_times(const vl3d_render_desc *desc, const uint8_t *baked, int32_t T_alloc, const float *homos,
                                const vl3d_baked_times *sel, const uint8_t *quad_keep, int32_t QH, int32_t QW, void *cull_scratch,
                                const vl3d_baked_out *out, vl3d_stream_t stream);
int vl3d_render_fwd_baked_pool_times(const vl3d_render_desc *desc, const int32_t *blocks, const uint8_t *pool, int32_t T_model,
                                     const float *homos, const vl3d_baked_times *sel, const uint8_t *quad_keep, int32_t QH, int32_t QW,
                                     uint32_t culled_rgba8, void *cull_scratch, const vl3d_baked_out *out, vl3d_stream_t stream);

/* Disparity (csrc/vl3d_render_disp.hip): the depth map beside the picture -- the reference's blend-weighted inverse view depth (MPV.py:385,
 * 463-466, MPI.py:493-494, 563-566) -- from the float clip, the baked clip and the baked pool, without a layer tensor.  Forward only, no host
 * synchronisation, kernels of their own: no colour entry above changes.
 *   The rule.  Planar geometry makes the inverse view depth of plane k under output pixel (x, y) AFFINE in the pixel:
 *         rho_k(x, y) = fmaf(rows[k][0], x + c, fmaf(rows[k][1], y + c, rows[k][2])),   x + c = (float)(col0 + x) + pixel_center, y likewise,
 *     rows (D, 3) device fp32, 4-byte aligned, formed on the host (render.depth_rows: row_k = K^-T r3 / (z_k + r3 . t), r3 the third column
 *     of the ref -> target rotation; any affine renormalisation of rho is folded into the rows, the kernel does not know about it).  With a_k
 *     the covered alpha of plane k as the colour forward of the same source forms it, T_0 = 1, T_k = prod_{j<k} (1 - a_j), w_k = a_k T_k:
 *         disp = sum_k w_k rho_k          alpha = sum_k w_k
 *     one step per plane, nothing contracted but the one spelt fmaf: w = a T; disp = fmaf(w, rho, disp); alpha += w; T *= 1 - a.  Sample
 *     position, hard cut, kept-quad test, tile-exact quad offset and tent weights are the float forward's own device functions: colour and
 *     depth agree on every pixel's coverage.  One output pixel and one frame per thread: a frame does not depend, in its last bit, on the
 *     run or path it is rendered in.  disp (N,H,W) fp32, N = desc->T; alpha (N,H,W) fp32 or NULL (not written).
 *   desc: the planar convention only -- VL3D_COORD_AFFINE, VL3D_BORDER_HARDCUT, uv_noise_seed = 0 (else VL3D_EUNSUPPORTED), variant = 0,
 *     D <= 128.
 *   vl3d_render_disp_fwd: frames frame0 .. frame0 + desc->T - 1 of a float clip (D, T_alloc, Hs, Ws, 4), fp32 or fp16, read in place as
 *     vl3d_render_fwd_frames reads it; homos (D, 3, 3).  act_order VL3D_ACT_POST (VL3D_ACT_BAKED: VL3D_EUNSUPPORTED): a_k = alpha_act(the
 *     bilinear blend of the four taps' alpha logits) * coverage, every alpha_act of the table with either dtype; rgb_act is not read and per
 *     tap only the alpha lane (4 or 2 bytes) is loaded.  quad_keep NULL = a dense model, else vl3d_render_fwd_frames's map, grid (negative:
 *     tile-exact layout), desc->cull_* window and vl3d_render_cull_scratch_bytes(desc) of scratch.
 *   vl3d_render_disp_baked / _baked_pool: the sources of vl3d_render_fwd_baked / _pool and their selection vl3d_baked_frames, unchanged --
 *     a run under homos (D, 3, 3) and rows (D, 3), or a path under homos (n_cams, D, 3, 3), rows (n_cams, D, 3), frame_cam, frame_t; scratch
 *     sizes as there.  a_k = the bilinear blend of the decoded alpha bytes (blend<3> of csrc/vl3d_baked_core.h, no activation) * coverage: the
 *     alpha written here has the bits of the float sink's alpha of the colour entry on the same call.  A tap in a pool block without storage
 *     reads the alpha byte of culled_rgba8; the pool's output has the bits of the clip entry on the unpacked texels; a path frame whose camera
 *     or frame is out of range stays unwritten.  There is no loop-time (vl3d_baked_times) form here: "RGB-D" below has it.
 *   VL3D_EINVAL, nothing launched, with the colour entries' messages: a NULL disp, rows, homos or source, a misaligned source, rows or
 *     output, D > 128, a run that leaves the clip, whatever check_baked_frames refuses, a bad quad grid. */
int vl3d_render_disp_fwd(const vl3d_render_desc *desc, const void *stack, int32_t frame0, int32_t T_alloc, const float *homos,
                         const float *rows, const uint8_t *quad_keep, int32_t QH, int32_t QW, void *cull_scratch, float *disp, float *alpha,
                         vl3d_stream_t stream);
int vl3d_render_disp_baked(const vl3d_render_desc *desc, const uint8_t *baked, int32_t T_alloc, const float *homos, const float *rows,
                           const vl3d_baked_frames *sel, const uint8_t *quad_keep, int32_t QH, int32_t QW, void *cull_scratch, float *disp,
                           float *alpha, vl3d_stream_t stream);
int vl3d_render_disp_baked_pool(const vl3d_render_desc *desc, const int32_t *blocks, const uint8_t *pool, int32_t T_model, const float *homos,
                                const float *rows, const vl3d_baked_frames *sel, const uint8_t *quad_keep, int32_t QH, int32_t QW,
                                uint32_t culled_rgba8, void *cull_scratch, float *disp, float *alpha, vl3d_stream_t stream);

/* RGB-D (csrc/vl3d_render_rgbd.hip): the picture of "Baked playback" AND the depth map of "Disparity" from ONE render launch -- one walk of
 * the planes, one fetch of the texels, one per-plane alpha -- for a run, a camera path and a path in loop time, which has no other depth
 * entry.  Forward only, no host synchronisation, kernels of their own: no entry above changes.
 *   The rule.  Per covered (pixel, plane) the colour statements of vl3d_render_fwd_baked (at a loop time: of vl3d_render_fwd_baked_times, every
 *     channel c_K = fmaf(f, b1_K - b0_K, b0_K), alpha included), nothing contracted, and with the SAME w = a T one more accumulator,
 *         disp = fmaf(w, rho_k, disp),   rho_k = fmaf(rows[k][0], x + c, fmaf(rows[k][1], y + c, rows[k][2]))        ("Disparity")
 *     rows (D, 3) for a run, (n_cams, D, 3) for a path, device fp32, 4-byte aligned (render.depth_rows; any normalisation folded in).
 *     Frame pairs per thread for a run of two or more frames, one output frame along a path, one output and two source frames at a loop time.
 *   Bit for bit: rgb and alpha are the float sink of the colour entry on the same call; frames its display sink; disp of a run or a path is
 *     vl3d_render_disp_baked(_pool) on the same call; a loop time with f == 0 has the bits of path frame (cam, t0), disp included, and equal
 *     texels in both frames give the same bits at any f; the pool has the bits of the clip entry on the unpacked texels; a frame does not
 *     depend on the run or path it is rendered in.
 *   Source, scratch and quad map: vl3d_render_rgbd_baked takes what vl3d_render_fwd_baked takes, vl3d_render_rgbd_baked_pool what
 *     vl3d_render_fwd_baked_pool takes; D <= 128.  Selection: exactly one of sel (vl3d_baked_frames: a run or a camera path) and times
 *     (vl3d_baked_times), the other NULL; a workgroup whose camera, frame or time is out of range returns before any load or store.
 *   Sink (vl3d_rgbd_out), exactly one of two.  FLOAT: rgb (N,H,W,3), alpha (N,H,W), disp (N,H,W) fp32, all three, 4-byte aligned; frames =
 *     depth16 = bg = NULL.  DISPLAY: frames / channels / bg by the rules of vl3d_baked_out's display sink, and depth16 (N,H,W) uint16, 2-byte
 *     aligned, every operation rounded on its own:
 *         depth16 = (uint16) trunc(65535 * min(max(disp, 0), 1))
 *     not divided by alpha and not composited over the background: a pixel no plane covers reads 0, which is far.  The normalisation of disp
 *     to [0, 1] is the caller's, folded into rows (render.depth_rows(normalise=(near, far))).  One two-byte store per pixel: a wave's 64
 *     levels are 128 contiguous bytes.
 *   VL3D_EINVAL, nothing launched: what the colour entry of the same source and vl3d_render_disp_baked(_pool) refuse, with their messages
 *     (a descriptor outside the planar convention is VL3D_EINVAL here, as in the colour entries); both or neither of sel / times; both sinks or
 *     neither; a float sink without disp (or without rgb or alpha); a display sink without depth16 (or without frames); a misaligned depth16,
 *     rgb, alpha, disp, rows or homos; a bg with the float sink. */
typedef struct vl3d_rgbd_out {
    float *rgb, *alpha, *disp;             /* the float sink: all three */
    uint8_t *frames;                       /* the display sink: vl3d_baked_out's frames ... */
    int32_t channels;
    const float *bg;                       /* ... its background: host float[3] or NULL ... */
    uint16_t *depth16;                     /* ... and the 16-bit depth (N,H,W) */
} vl3d_rgbd_out;                           /* 56 bytes */
int vl3d_render_rgbd_baked(const vl3d_render_desc *desc, const uint8_t *baked, int32_t T_alloc, const float *homos, const float *rows,
                           const vl3d_baked_frames *sel, const vl3d_baked_times *times, const uint8_t *quad_keep, int32_t QH, int32_t QW,
                           void *cull_scratch, const vl3d_rgbd_out *out, vl3d_stream_t stream);
int vl3d_render_rgbd_baked_pool(const vl3d_render_desc *desc, const int32_t *blocks, const uint8_t *pool, int32_t T_model, const float *homos,
                                const float *rows, const vl3d_baked_frames *sel, const vl3d_baked_times *times, const uint8_t *quad_keep,
                                int32_t QH, int32_t QW, uint32_t culled_rgba8, void *cull_scratch, const vl3d_rgbd_out *out,
                                vl3d_stream_t stream);

/* A viewer package's atlases -> the baked pool (csrc/vl3d_pool_from_atlas.hip; baked.open_viewer_package).  A package IS a baked pool in another
 * order: RGBA8 tiles of th x tw texels of the kept quads, static tiles once (static_atlas, As_h x As_w texels, row-major grid of
 * As_w / tw tiles per row), dynamic tiles per frame (dyn_atlas, Ad_h x Ad_w: the atlas of frame `frame`), culled quads absent.  The
 * destination is the pool of the TILE-EXACT layout of the quad maps (Hs = QH th, Ws = QW tw) behind its block table `blocks`
 * [D][ceil(Hs/8)][ceil(Ws/8)] (vl3d_render_fwd_baked_pool above).  tile_src [D][QH][QW] int32 (device): -1 (culled) | k << 1 | dynamic, k the
 * tile's index in its atlas.  One call writes frame `frame`: a static block (entry & 1 == 0) only when frame == 0, a dynamic block at slot +
 * frame; each of a written block's 64 texels (y, x) is 0 past the plane, culled_rgba8 inside a culled tile, else the tile's texel
 * atlas[(k / gw) th + y % th][(k % gw) tw + x % tw] -- a static tile inside a dynamic block in every frame.  One wave per block, one lane
 * per texel: 64 dwords stored contiguously.  A block without storage (-1) returns before any other load.
 * Bounds.  A k outside its atlas grid reads culled_rgba8 (the kernel compares it with the grid the sizes give; the wrapper range-checks
 * the host copy of tile_src before it uploads it); an atlas pointer may be NULL with sizes 0 x 0 (a package without static, or without
 * dynamic, quads).  The table is trusted as packed.PackedLayout builds it for T frames: every stored slot (+ T - 1 for a dynamic block) lies
 * inside the pool.  VL3D_EINVAL, nothing launched: D, T, th, tw, QH, QW < 1, Hs != QH th, Ws != QW tw, frame outside [0, T), a NULL or
 * misaligned (4 bytes) pointer, an atlas size that is not a multiple of the tile size, D * blocks per plane > 2^31 - 1. */
int vl3d_pool_from_atlas_rgba8(int32_t D, int32_t T, int32_t Hs, int32_t Ws, int32_t th, int32_t tw, int32_t QH, int32_t QW,
                               const int32_t *blocks, const int32_t *tile_src, const uint8_t *static_atlas, int32_t As_h, int32_t As_w,
                               const uint8_t *dyn_atlas, int32_t Ad_h, int32_t Ad_w, int32_t frame, uint32_t culled_rgba8, uint8_t *pool,
                               vl3d_stream_t stream);

/* Trimming a baked pool (csrc/vl3d_baked_trim.hip; baked.BakedPool.trimmed; docs/kernels/K9_baked_playback.md "Trimming the pool").  The pool
 * stands for the clip [D][T][Hs][Ws] RGBA8 its table gives (a block without storage reads culled_rgba8).  Over the in-plane texels of that clip:
 * A = the largest alpha byte of the T frames; show = some texel of the 3 x 3 neighbourhood (clipped to the plane) has A > 0; moves = show and the
 * texel's four bytes differ between some frame and frame 0.  A stored block none of whose texels shows needs no storage when the alpha byte of
 * culled_rgba8 is 0; a dynamic block that is kept and none of whose texels moves is one static block holding frame 0.
 * vl3d_baked_trim_classify: two launches, one wave per block of the table, one lane per texel.  The first writes the texel flags (bit 0 A > 0,
 * bit 1 "differs from frame 0") as a [D][Hs][Ws] byte map into `scratch` (vl3d_baked_trim_scratch_bytes(D, Hs, Ws) bytes: the map, rounded up to
 * 256), the second block_slots [D][ceil(Hs/8)][ceil(Ws/8)] int32 = the block's new slot count 0 | 1 | T and texel_class [D][Hs][Ws] bytes (bit 0
 * show, bit 1 moves).  Texels of a ragged block past the plane's last row / column are not read into either map and write nothing.
 * vl3d_baked_trim_move: new_blocks is the table of the exclusive scan of block_slots (-1 | start << 1 | (count > 1)), which the caller forms;
 * one wave per (block, frame) copies the 256 bytes of every slot the new table keeps from pool to new_pool (frame 0 of a block that became static).
 * Bounds.  The table is trusted as packed.PackedLayout builds it for T frames (as the render entries trust it).  What cannot be crossed whatever it
 * holds: the block index is below D * ceil(Hs/8) * ceil(Ws/8); an entry -1 is never dereferenced, and an entry whose slots (1, or T for a dynamic
 * block) would end past n_slots / new_n_slots is read as -1; neighbour reads of the flag map are clamped to the plane; a block of the new table
 * that is dynamic where the old one is not is not copied.  No LDS, no atomics, one writer per byte: bit-for-bit deterministic; every launch on
 * `stream`.  VL3D_EINVAL, nothing launched: a NULL pointer (a pool may be NULL with 0 slots), D, T, Hs, Ws < 1, D > 65535, blocks per plane * T
 * > 2^31 - 5, a misaligned (4 bytes) table or pool, scratch_bytes below the size function's value, texel_class == scratch, new_pool == pool. */
int64_t vl3d_baked_trim_scratch_bytes(int32_t D, int32_t Hs, int32_t Ws);
int vl3d_baked_trim_classify(int32_t D, int32_t T, int32_t Hs, int32_t Ws, const int32_t *blocks, const uint8_t *pool, int64_t n_slots,
                             uint32_t culled_rgba8, void *scratch, int64_t scratch_bytes, int32_t *block_slots, uint8_t *texel_class,
                             vl3d_stream_t stream);
int vl3d_baked_trim_move(int32_t D, int32_t T, int32_t Hs, int32_t Ws, const int32_t *blocks, const uint8_t *pool, int64_t n_slots,
                         const int32_t *new_blocks, uint8_t *new_pool, int64_t new_n_slots, vl3d_stream_t stream);

/* Backward of the above w.r.t. the stack (geometry is not differentiated: MPV.py:354).
 * rgb/alpha are the saved forward outputs; grad_alpha may be NULL (treated as 0).
 * grad_alpha_sums (optional): (T,H,W,2) gradient w.r.t. alpha_sums of the forward.
 * grad_stack (D,T,Hs,Ws,4) is overwritten; it has the dtype of the stack (fp32, or fp16 for stack_dtype == VL3D_F16 -- the
 * cfg5 shards only fit with an 8-byte gradient texel).
 * scratch: caller-owned device buffer of vl3d_render_bwd_scratch_bytes(desc) bytes (plan written and read on
 * `stream`, no host sync); with scratch == NULL the universal global-atomics kernel is used.
 * desc->variant bits 0-3 (the rules, in order, with their measurements: choose_bwd(), csrc/vl3d_render_bwd_choice.h):
 *   0  auto: the owner-computes kernels (LDS-staged, no atomics) when the on-device feasibility plan allows, the atomics kernel
 *      otherwise.  T >= 2, dense, sigmoid / sigmoid: two frames per thread -- in 64 x 12-pixel regions without layer regularisers where
 *      the stack is no larger than the frame (+7 %) along one axis at least, in 32 x 16 regions with them (not under VL3D_COORD_UTILS_MPI).
 *      T = 1, no regularisers, the shipped planar convention (affine, hardcut, post, sigmoid / sigmoid, fp32): one frame per thread in flat
 *      64 x 8 regions.  A quad map under VL3D_GRAD_CULLED_UNWRITTEN, same convention: one frame per thread in 32 x 16 regions.  Everything
 *      else: one frame per thread in 64 x 16 regions.
 *   1  the atomics kernel alone (also: scratch NULL or short, uv_noise_seed != 0)
 *   2  one frame per thread in flat 64 x 8 regions at any T (shipped planar convention, dense, no regularisers; = 3 elsewhere)
 *   3  one frame per thread in 64 x 16 regions, the owner table built one texel per thread
 *   4  = 3 with the 3x3 gather everywhere (reference for the 2x2 gather of no-minification tiles, which must equal it bit for bit)
 *   5  one frame per thread in 32 x 16 regions (shipped planar convention; = 3 elsewhere)
 *   6 / 7  two frames per thread in 32 x 16 / 64 x 12 regions wherever 0 takes frame pairs WITHOUT regularisers; = 3 elsewhere.  7 is the
 *      64 x 12 kernel that reads the per-call owner table (one uint16 per plane texel in `scratch`)
 *   8  two frames per thread in 64 x 12 regions WITHOUT the owner table wherever 0 takes frame pairs without regularisers: every gather
 *      thread computes its texel's owner pixel itself, the table region of `scratch` is not touched; = 0 elsewhere.  vl3d_render_bwd_choice
 *      reports VL3D_BWD_PAIR12, 64 x 12 for 7 and 8 alike.  0 takes 8's kernel for fp32 stacks outside VL3D_COORD_UTILS_MPI and 7's otherwise (as measured:
 *      BWD_PAIR12_AUTO_OWNERLESS_*, csrc/vl3d_render_bwd_choice.h)
 *   every other value = 3.  All of them produce the same gradient bits.
 * vl3d_render_bwd_mask: 3 / 4 the 64 x 16 regions, 1 atomics, every other value flat 64 x 8 regions (its default).  vl3d_render_bwd_adam: a
 * dense model (variant 0 only) rides the 32 x 16 frame pairs; a tile-culled one 32 x 16 one-frame regions, 64 x 16 with variant 3.
 * quad_keep NULL = a dense model (QH, QW are not read), else the forward's quad map and grid ("Tile culling" below): a sample in a culled
 * quad passes no gradient; the plan of the culled backward lives in the same scratch. */
int64_t vl3d_render_bwd_scratch_bytes(const vl3d_render_desc *desc);
int vl3d_render_bwd(const vl3d_render_desc *desc, const void *stack, const float *homos, const uint8_t *quad_keep, int32_t QH, int32_t QW,
                    const float *rgb, const float *alpha, const float *grad_rgb, const float *grad_alpha, const float *grad_reg,
                    const void *reg_state, const float *grad_alpha_sums, float *grad_stack, void *scratch, int64_t scratch_bytes,
                    vl3d_stream_t stream);

/* Stage 1's view-dependent colour head, rgb_mlp_type = "rgb_sh" (csrc/vl3d_render_sh.hip; docs/kernels/K7_stage1.md, "the view-dependent colour head").  Replaces MPI.py:512-513,
 * 526-537 inside the render MPI.py:452-594: per-pixel ray directions into SphericalHarmoic_RGB (utils_mpi.py:50-61) with the degree-1 basis of
 * eval_sh_bases (utils_mpi.py:365-383), and its autograd.
 *   stack    : (D, 1, Hs, Ws, 4)     (R0, G0, B0, alpha logit): coefficient k = 0 of every colour and the alpha, as vl3d_render_fwd reads it
 *   stack_sh : (D, 1, Hs, Ws, 3, 4)  stack_sh[..., k - 1, c] = coefficient k = 1..3 of colour c; lane 3 is reserved: 0, never read into a value
 *   homos    : (D, 3, 3)             as vl3d_render_fwd
 *   ray_m    : device float[9], row-major M = inverse(E)[:3,:3] inverse(K) -- E the ref -> target extrinsic, K the intrinsics of the call
 * Per output pixel with INTEGER frame indices (x, y) = (col0 + column, row0 + row) (utils.py:182-193: no half pixel, whatever pixel_center says):
 *     d = normalize(M (x, y, 1)^T),   b = (C0, -C1 d_y, C1 d_z, -C1 d_x),   C0 = 0.28209479177387814, C1 = 0.4886025119029199
 * Per plane: the taps, hard cut, kept-quad test and tent weights of vl3d_render_fwd's planar convention (the same device functions);
 *     pre_c = sum_k b_k sample(coef_{c,k}),  pre_a = sample(alpha)  (contracted per tap, before the tent weights: the contraction is linear),
 *     rgba = (rgb_act(pre_rgb), alpha_act(pre_a)) x coverage, composited front to back as vl3d_render_fwd does.  With stack_sh = 0, alpha and
 *     alpha_sums hold the bits of vl3d_render_fwd.  M and 2 M give the same bits.  A wave skips a plane that covers none of its 64 pixels.
 * Forward writes rgb (1,H,W,3), alpha (1,H,W) and alpha_sums (1,H,W,2; may be NULL).  Backward: rgb / alpha the saved outputs, grad_alpha and
 *     grad_alpha_sums may be NULL; grad_stack and grad_stack_sh are overwritten -- cleared by the entry, then summed with global float atomics
 *     (per tap with tent weight w: d/d coef_{c,k} += w b_k g_pre_c, d/d alpha += w g_pre_a, g_pre = act'(pre) g_layer; a wave transposes its
 *     pixels' 16-float texel records through LDS so that one atomic instruction carries whole records of 4 pixels), so the gradient is NOT
 *     bit-reproducible between runs; lane 3 of grad_stack_sh and every texel no covered sample reads are exactly 0.
 * Accepted: T = 1, VL3D_F32, (VL3D_COORD_AFFINE, VL3D_BORDER_HARDCUT, VL3D_ACT_POST), every pair of the activation table, D <= 128; quad_keep NULL
 *     (QH, QW not read) or a map [D][QH][QW] with a POSITIVE grid and desc->cull_* = 0.  VL3D_EUNSUPPORTED: another T, dtype or convention,
 *     uv_noise_seed != 0, the tile-exact (negative) grid, a cull window.  VL3D_EINVAL: variant != 0, non-positive dims, D > 128, a plane of
 *     2^28 texels or more, a NULL pointer, stack / stack_sh / their gradients not 16-byte aligned, any other pointer not 4-byte aligned.  Nothing
 *     is launched after a refusal. */
int vl3d_render_sh_fwd(const vl3d_render_desc *desc, const float *stack, const float *stack_sh, const float *homos, const float *ray_m,
                       const uint8_t *quad_keep, int32_t QH, int32_t QW, float *rgb, float *alpha, float *alpha_sums, vl3d_stream_t stream);
int vl3d_render_sh_bwd(const vl3d_render_desc *desc, const float *stack, const float *stack_sh, const float *homos, const float *ray_m,
                       const uint8_t *quad_keep, int32_t QH, int32_t QW, const float *rgb, const float *alpha, const float *grad_rgb,
                       const float *grad_alpha, const float *grad_alpha_sums, float *grad_stack, float *grad_stack_sh, vl3d_stream_t stream);

/* Camera gradients (csrc/vl3d_render_cam.hip): d loss / d homos of vl3d_render_fwd's picture and of vl3d_warp_fwd's -- what the reference's
 * autograd passes through grid_sample's grid to `homos` (utils_mpi.py:159-176) and on to extrinsics and intrinsics (compute_homography).
 * Per output pixel (u, v) = (col0 + x + c, row0 + y + c), c = desc->pixel_center, plane d, frame t: (X, Y, Z) = H_d (u, v, 1),
 * tx = sx X / Z + ox, ty = sy Y / Z + oy (VL3D_COORD_UTILS_MPI: sx = (Ws - 1) / Ws, sy = (Hs - 1) / Hs, ox = oy = 0); x0 = floor(tx), fx = tx - x0:
 * floor carries no gradient, fx does (ATen's grid_sample rule); a tap outside the texture counts as 0, as in the forward:
 *     ds/dtx = (S10 - S00)(1 - fy) + (S11 - S01) fy,   ds/dty = (S01 - S00)(1 - fx) + (S11 - S10) fx      per channel
 * (the taps are the activated texels under VL3D_ACT_PRE).  g_pre, the gradient with respect to the sampled values of (pixel, plane, frame), is
 * the quantity vl3d_render_bwd scatters with the tent weights -- the same device functions decide coverage, kept quads, the composite
 * backward from the saved rgb / alpha and act' --, zero where the plane does not cover the pixel; coverage and quad membership are step
 * functions and carry no gradient.  With g_tx = sum_t sum_c g_pre_c ds_c/dtx, a = g_tx sx / Z, b = g_ty sy / Z, e = -(g_tx sx X + g_ty sy Y) / Z^2:
 *     grad_homos[d] = sum over pixels of (a, b, e)^T (u, v, 1)         [D][3][3], overwritten
 * No float atomics: sums over the wave's lanes, then the workgroup's waves, one [D][9] partial per workgroup in `scratch`, and a finish kernel
 * that adds the partials in a fixed order in fp64.  Two calls give identical bits.  grad_alpha may be NULL.
 * Accepted: VL3D_F32 stacks, any T >= 1, D <= 128; (VL3D_COORD_AFFINE, VL3D_BORDER_HARDCUT, VL3D_ACT_POST) and (VL3D_COORD_UTILS_MPI,
 *     VL3D_BORDER_ZEROS, VL3D_ACT_PRE); every pair of the activation table; row0 / col0 windows; quad_keep NULL (QH, QW not read) or a map
 *     [D][QH][QW] with a POSITIVE grid and desc->cull_* = 0.  VL3D_EUNSUPPORTED: fp16 stacks, any other convention (VL3D_COORD_AFFINE_PLANES,
 *     VL3D_ACT_BAKED included), the tile-exact (negative) grid, a cull window, uv_noise_seed != 0.  VL3D_EINVAL: variant != 0, non-positive dims,
 *     D > 128, a plane of 2^28 texels or more, a NULL pointer, stack not 16-byte aligned, any other pointer not 4-byte aligned, scratch_bytes
 *     below vl3d_render_bwd_homos_scratch_bytes(desc).  Nothing is launched after a refusal.
 * vl3d_warp_bwd_homos: the same for vl3d_warp_fwd (images (N, C, Hs, Ws), grad_out (N, C, h, w), c = 0, the utils_mpi coordinates): g_pre is
 *     the upstream gradient of image n itself; grad_homos [N][3][3], overwritten.  VL3D_EINVAL as vl3d_warp_bwd, plus alignment and scratch. */
int64_t vl3d_render_bwd_homos_scratch_bytes(const vl3d_render_desc *desc);
int vl3d_render_bwd_homos(const vl3d_render_desc *desc, const void *stack, const float *homos, const uint8_t *quad_keep, int32_t QH, int32_t QW,
                          const float *rgb, const float *alpha, const float *grad_rgb, const float *grad_alpha,
                          float *grad_homos /* [D][3][3], overwritten */, void *scratch, int64_t scratch_bytes, vl3d_stream_t stream);
int64_t vl3d_warp_bwd_homos_scratch_bytes(int32_t N, int32_t h, int32_t w);
int vl3d_warp_bwd_homos(int32_t N, int32_t C, int32_t Hs, int32_t Ws, int32_t h, int32_t w, const float *homos, const float *images,
                        const float *grad_out, float *grad_homos /* [N][3][3] */, void *scratch, int64_t scratch_bytes, vl3d_stream_t stream);

/* Camera normal equations (csrc/vl3d_render_cam_normal.hip): the Gauss-Newton system of the photometric residual r = rgb - target of
 * vl3d_render_fwd's picture in P camera parameters theta, for Levenberg-Marquardt steps on the host (videoloop3d_amd/poses.py).  The kernel
 * knows nothing about poses: the host chain supplies the tangent homographies dhomos [P][D][3][3], dhomos[k] = dH / d theta_k, 1 <= P <= 8.
 * Per output pixel (u, v) (window and pixel centre as in the camera gradient), plane d, parameter k: (X, Y, Z) = H_d (u, v, 1),
 * (dX, dY, dZ)_k = dhomos[k][d] (u, v, 1),
 *     dtx_{d,k} = sx (dX_k - (X / Z) dZ_k) / Z,   dty_{d,k} = sy (dY_k - (Y / Z) dZ_k) / Z        (sx, sy as in the camera gradient)
 * Per frame t and colour channel c: g_pre^(c) is the composite backward with upstream gradient e_c (alpha gradient 0), by the device functions
 * of the camera gradient -- the (S - P) rcp(1 - a) form with its look-ahead, S_c = rgb_c the saved forward picture; coverage and quad
 * membership carry no gradient; ds/dtx, ds/dty are the tent-slope contractions of the camera gradient:
 *     J[t,p,c,k] = sum_d sum_ch g_pre^(c)_{d,ch} (ds_ch/dtx dtx_{d,k} + ds_ch/dty dty_{d,k}),     r[t,p,c] = rgb - target
 *     out = A [P][P] = sum_{t,p,c} w J_k J_l (symmetric, both triangles written),  b [P] = sum w J_k r,  cost = sum w r^2      float64, overwritten
 * with w = weight[t,p] (T,H,W), 1 if weight is NULL.  No float atomics: sums over rows of 16 lanes, LDS slots with one writer each, one
 * fp64 partial per workgroup in `scratch`, a finish kernel that adds the partials in a fixed order in fp64.  Two calls give identical bits.
 * Accepted: exactly what vl3d_render_bwd_homos accepts; everything it refuses is refused here with the same codes.  In addition VL3D_EINVAL:
 *     P < 1 or P > 8, a NULL dhomos / rgb / target / out, out or scratch not 8-byte aligned, scratch_bytes below
 *     vl3d_render_cam_normal_scratch_bytes(desc, P).  Nothing is launched after a refusal, and `out` is not written. */
int64_t vl3d_render_cam_normal_scratch_bytes(const vl3d_render_desc *desc, int32_t P);
int vl3d_render_cam_normal(const vl3d_render_desc *desc, const void *stack, const float *homos, const float *dhomos, int32_t P,
                           const uint8_t *quad_keep, int32_t QH, int32_t QW, const float *rgb, const float *target, const float *weight,
                           double *out /* double[P*P + P + 1] */, void *scratch, int64_t scratch_bytes, vl3d_stream_t stream);

/* Camera registration (csrc/vl3d_render_cam_register.hip): the normal equations above for a target that is a CAPTURED clip of the view, not the
 * model's own picture frame for frame -- the same loop started at an unknown time, exposed differently.  C[t,p,c] is the saved forward picture
 * `rgb`, J[t,p,c,k] the per-pixel Jacobian exactly as vl3d_render_cam_normal forms it (the same device functions, coverage rules and tent
 * slopes), g = exp(log_gain), beta = bias: the point at which the system is evaluated.
 *   mode = VL3D_CAM_PER_FRAME:      r[t,p,c] = g C + beta - I[t,p,c];   column k < P: g J[t,p,c,k];  target (T,H,W,3), weight (T,H,W) or NULL
 *   mode = VL3D_CAM_LONG_EXPOSURE:  Cm[p,c] = (1 / T) sum_t C,  Jm[p,c,k] = (1 / T) sum_t J,  r[p,c] = g Cm + beta - I[p,c];  column k < P: g Jm;
 *                                   target (H,W,3) -- the temporal mean of the clip --, weight (H,W) or NULL
 *   photo = 1: two more unknowns, the log gain and the bias: column P is g C (g Cm), column P + 1 is 1.  photo = 0: (log_gain, bias) still
 *              shape the residual and the columns, but are not unknowns.
 *     out = A [Q][Q] = sum w col_k col_l (both triangles written),  b [Q] = sum w col_k r,  cost = sum w r^2,   Q = P + 2 photo;
 *     double[Q*Q + Q + 1], overwritten.
 * A long exposure of a clip equals the loop's only when the clip spans whole loop periods: a caveat of the method, not of the kernel.
 * The reduction is vl3d_render_cam_normal's: no float atomics, one fp64 partial per workgroup in `scratch`, a finish kernel that adds them in a
 * fixed order; two calls give identical bits; at T = 1 the two modes give identical bits.
 * Accepted: exactly what vl3d_render_cam_normal accepts; everything it refuses is refused here with the same codes.  In addition VL3D_EINVAL:
 *     mode or photo outside {0, 1}, a non-finite log_gain or bias (or exp(log_gain) not a finite float), P < 1 or P > 8, a NULL or misaligned
 *     pointer, scratch_bytes below vl3d_render_cam_register_scratch_bytes(desc, P, photo) (0 for arguments it refuses).  Nothing is launched
 *     after a refusal, and `out` is not written. */
enum { VL3D_CAM_PER_FRAME = 0, VL3D_CAM_LONG_EXPOSURE = 1 };
int64_t vl3d_render_cam_register_scratch_bytes(const vl3d_render_desc *desc, int32_t P, int32_t photo);
int vl3d_render_cam_register(const vl3d_render_desc *desc, const void *stack, const float *homos, const float *dhomos, int32_t P,
                             const uint8_t *quad_keep, int32_t QH, int32_t QW, const float *rgb, const float *target, const float *weight,
                             int32_t mode, int32_t photo, float log_gain, float bias,
                             double *out /* double[Q*Q + Q + 1] */, void *scratch, int64_t scratch_bytes, vl3d_stream_t stream);

/* Which kernel a backward call runs, without running it: the value the entry points themselves compute (the same two functions, no device
 * touched, nothing enqueued).  entry: which entry point; has_quad_keep / has_reg_grads (grad_reg or grad_alpha_sums non-NULL) / scratch_bytes:
 * as the call would pass them (scratch_bytes 0 = scratch NULL); fused_step: vl3d_render_bwd_adam (entry VL3D_BWD_ENTRY_ADAM) only.  Refusals
 * are the entry's own descriptor refusals (VL3D_EINVAL / VL3D_EUNSUPPORTED) -- all but two it cannot see: the quad grid's rules (QH, QW are
 * not passed) and an activation pair its convention is not built for.  width x rows: the workgroup's region, 0 x 0 for VL3D_BWD_ATOMICS;
 * a feasible plan is the device's to decide -- family says what runs when it is. */
enum { VL3D_BWD_ENTRY_RENDER = 0, VL3D_BWD_ENTRY_MASK = 1, VL3D_BWD_ENTRY_ADAM = 2 };
enum { VL3D_BWD_ATOMICS = 0, VL3D_BWD_TILE = 1, VL3D_BWD_PAIR = 2, VL3D_BWD_PAIR12 = 3 };
typedef struct vl3d_bwd_choice {
    int32_t family;                        /* VL3D_BWD_*: atomics only | one frame per thread | frame pairs | frame pairs, 64 x 12 kernel */
    int32_t width, rows;
    int32_t reg, mask, adam, cull, f16;    /* the instantiation: regularisers' build, fifth channel, fused step, quad map, fp16 texels */
    int32_t owner4;                        /* the owner table is built four texels per thread */
    int32_t gather9;                       /* the 3x3 gather everywhere (variant 4) */
} vl3d_bwd_choice;
int vl3d_render_bwd_choice(const vl3d_render_desc *desc, int32_t entry, int32_t has_quad_keep, int32_t has_reg_grads, int64_t scratch_bytes,
                           int32_t fused_step, vl3d_bwd_choice *out);

/* Tile culling (MPI.py:288-442 "Tile Culling Algorithm": stage 2 renders only the quads that survived).  quad_keep is a device
 * byte map [D][QH][QW] over the cells of each plane's vertex grid ((Ws-1)/QW x (Hs-1)/QH texels per quad), 1 = the quad exists.
 * A sample that falls into a culled quad of a plane is NOT COVERED by that plane (the reference's mesh has no face there):
 * it contributes nothing and passes no gradient, whatever the texels hold; its layer value for the smoothness regularisers
 * is 0 like any uncovered pixel (MPV.py:441).  On top of that rule, work is skipped where a whole workgroup sees no kept
 * quad of a plane (forward: a 64-bit plane mask per workgroup walked with scalar bit scans; backward: a flag in the tile's
 * window record -- no sweep, no barrier, zeros stored to the texels it owns), which changes no result.  D <= 128.
 * cull_scratch: vl3d_render_cull_scratch_bytes(desc) bytes (forward plan, rebuilt every call, no host sync); the backward
 * keeps its plan in its own scratch. */
/* Tile-exact layout (round 6).  `sparsify_faces` cuts every kept quad out of the atlas as a tile WITH ITS OWN border row / column (MPI.py:380-418:
 * neighbouring tiles hold two copies of their common border samples), every face's UVs span exactly its tile (gen_quad_uvs, MPI.py:403-418;
 * sampled by MPV.py:394-427 / MPI.py:497-536), and stage 2 trains the two copies APART -- a static tile's copy is one texture, its dynamic
 * neighbour's copy moves per frame.  A stack on which neighbouring quads SHARE their border texels (the layout above) cannot hold such a
 * checkpoint.  Passing a NEGATIVE quad grid (-QH, -QW) to an entry that takes a quad map selects the tile-exact layout instead:
 *   - a plane is QH x QW tiles of th x tw texels, th = Hs / QH, tw = Ws / QW (whole tiles of at least 2 x 2 texels; with desc->cull_*: of the
 *     cull_Hs x cull_Ws plane the stack is a window of -- the window itself need not be tile aligned); texel (y, x) belongs to quad
 *     (y / th, x / tw) and to no other: its class (culled / static / dynamic) is that quad's;
 *   - desc->sx, sy, ox, oy map a plane pixel to the LATTICE coordinate L (quads sharing borders: a quad spans tw - 1 of them, quad q =
 *     floor(L / (tw - 1))); the sample's texel coordinate is L + q -- position L - q (tw - 1) in [0, tw - 1] inside tile q, whose first texel
 *     is q tw -- so its bilinear taps never leave its own tile with a non-zero weight: grid_sample(align_corners=True) on the reference's
 *     atlas between the tile's corner texel centres.  With a window, ox / oy are reduced by the window's texel origin as usual.
 *   - everything else (hard cut at the plane's extent, culled quads uncovered, hit-slot regularisers, owner-computes backward, the fused
 *     optimiser step, packed pools, add_uv_noise jittering the TILE coordinate) is unchanged: the layout is a piecewise translation of the
 *     texel coordinate.  VL3D_COORD_AFFINE + VL3D_BORDER_HARDCUT only (the reference has tiles on the planar MPV / MPI path only).
 * Pinned by golden G19 (tests/golden/make_golden_r06.py: the reference's own forward on a checkpoint whose border copies differ). */
int64_t vl3d_render_cull_scratch_bytes(const vl3d_render_desc *desc);

/* Row bands with PER-PLANE source windows (videoloop3d_amd/dist.py plan_plane_bands; csrc/vl3d_render_plane_rows.hip).  The stack is a
 * rank's local (D, T, R, Ws, 4) rows: local row r of plane d is plane row plane_row0[d] + r (plane_row0: device int32[D]).  desc is the
 * descriptor of the same band rendered from the full stack: desc->Hs is the TRUE plane height, (row0, col0) the band's window, and the
 * texel coordinate is computed exactly as the full-frame kernels compute it -- the plane's integer origin is subtracted from the base tap's
 * row index only, so the bilinear weights are the full-frame bits and the hard cut is at the true plane border.  Rows a band pixel's taps
 * cannot reach (past a plane's own window) are padding: the backward leaves them 0.  The caller's windows must hold every row the band's
 * taps reach (the planner's corner argument + margin); the kernels clamp the local tap row into [0, R - 2] so that a wrong table cannot
 * address outside the allocation.  Built for the planar MPV convention (VL3D_COORD_AFFINE, VL3D_BORDER_HARDCUT, VL3D_ACT_POST,
 * sigmoid / sigmoid), fp32 and fp16 stacks; no regularisers, tile culling or uv noise.  2 <= R <= Hs.
 * The backward is the dense render's owner-computes frame-pair path (no atomics, deterministic bits): its plan, tile windows and owner
 * table live in `scratch`, vl3d_render_plane_rows_scratch_bytes(desc, R) bytes, written and read by the call.  Geometry outside that
 * path's preconditions (or scratch == NULL) takes the atomics sweep on a cleared gradient, as vl3d_render_bwd does. */
int vl3d_render_fwd_plane_rows(const vl3d_render_desc *desc, const void *stack, const int32_t *plane_row0, int32_t R, const float *homos,
                               float *rgb, float *alpha, vl3d_stream_t stream);
int64_t vl3d_render_plane_rows_scratch_bytes(const vl3d_render_desc *desc, int32_t R);
int vl3d_render_bwd_plane_rows(const vl3d_render_desc *desc, const void *stack, const int32_t *plane_row0, int32_t R, const float *homos,
                               const float *rgb, const float *alpha, const float *grad_rgb, const float *grad_alpha, void *grad_stack,
                               void *scratch, int64_t scratch_bytes, vl3d_stream_t stream);

/* Static tiles of a tile-culled VIDEO stack (MPV.py:235-288: one static atlas shared by all frames).  In place on the stack
 * gradient (D,T,Hs,Ws,4): texels that only static quads can read get the sum over the T frames in every frame (the T copies
 * then stay one texture under any optimiser), texels no kept quad can read get 0, texels a dynamic quad can read are left
 * alone.  quad_keep / quad_dyn: device byte maps [D][QH][QW].  mode bit 0: the gradient comes from the culled render
 * (vl3d_render_bwd with a quad map), which leaves exactly 0 in culled texels -- they are not rewritten.  mode bit 1: the consumer is
 * vl3d_adam_step_tiles with the same quad_dyn, which reads a static texel's gradient from frame 0 only -- the sum is written
 * to frame 0 alone (the other frames keep their per-frame values and must not be used). */
int vl3d_tie_static_grad(int32_t D, int32_t T, int32_t Hs, int32_t Ws, const uint8_t *quad_keep, const uint8_t *quad_dyn,
                         int32_t QH, int32_t QW, float *grad, int32_t mode, vl3d_stream_t stream);

/* torch.optim.Adam step (no amsgrad, no weight decay; MPV.py:199-214) on a stack parameter (D,T,Hs,Ws,4), in place on param /
 * exp_avg / exp_avg_sq, restricted to the texels a kept quad can read (quad_keep NULL: all texels).  Culled texels have zero
 * gradient and zero moments for ever, so skipping them is exact; `step` is the 1-based step count of this update.
 * (QH, QW) negative: the tile-exact layout ("Tile-exact layout" above; also for vl3d_tie_static_grad and the vl3d_adam_window_* family).
 * quad_dyn (optional, with quad_keep): texels only static quads can read are ONE parameter with T identical copies -- the
 * update is computed once from frame 0 (gradient = the frame sum vl3d_tie_static_grad leaves there; moments live in frame 0)
 * and the new value is written to all T copies. */
int vl3d_adam_step_tiles(int32_t D, int32_t T, int32_t Hs, int32_t Ws, const uint8_t *quad_keep, const uint8_t *quad_dyn, int32_t QH, int32_t QW,
                         float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float lr, float beta1, float beta2,
                         float eps, int64_t step, vl3d_stream_t stream);

/* Crop-aware Adam for the DENSE stack (csrc/vl3d_optim.hip; the optimiser of train_3dvid.py:263-290 / MPV.py:199-214).  A training
 * iteration renders one crop, so only the texels of the crop's parallax window (vl3d_adam_window's y0, x0, wh, ww; aligned to
 * vl3d_adam_window_tile()-texel tiles, or ending at the plane border) receive a gradient; the zero-gradient Adam steps of all
 * other texels (m <- b1 m, v <- b2 v, p <- p - lr_t m^/(sqrt(v^) + eps)) are deferred and replayed exactly, per tile, when a tile is
 * next needed.  last_step: device int32 [D][ceil(Hs/16)][ceil(Ws/16)], the step each tile is current for (0 initially).
 * hist: device float2 [steps+1], entry t = (lr_t / (1 - beta1^t), sqrt(1 - beta2^t)) as vl3d_adam_step_scalars computes them.
 * Round 6: the step functions (vl3d_adam_window_step, vl3d_render_bwd_adam) WRITE row `step` themselves from the struct's lr / betas /
 * step, behind the update, in the launch that marks the tiles (the table is `const` for every reader; a caller that also fills the row
 * writes the same two floats).  The caller sizes the table (step < its length) and keeps rows 0 .. step intact.
 *   vl3d_adam_window_catchup: the window's parameters as of step `upto` (steps last_step+1 .. upto replayed with g = 0).  With
 *     compact != NULL they are written to the compact (D,T,wh,ww,4) buffer the render then reads and the stack is left untouched;
 *     with compact == NULL (a flush) they are written back and the tiles marked current.
 *   vl3d_adam_window_step: replays the missed steps of the window's tiles up to step-1, then the Adam update of step `step` from the
 *     compact gradient (D,T,wh,ww,4), writes (p, m, v) and marks the tiles.  Everything outside the window stays deferred.
 * A catch-up with the full plane as the window makes the whole stack current (checkpoints, lod, evaluation renders).
 * Tile-culled models (quad_keep / quad_dyn != NULL, device byte maps [D][QH][QW]): culled texels are no parameters (the compact copy
 * shows them as (0, 0, 0, culled_alpha)); a texel only static quads can read is ONE parameter stored in frame 0 -- the compact copy
 * shows it in every frame, the step sums its compact gradient over the frames and writes frame 0 only; mirror_static bit 0 makes a
 * catch-up refresh the other frames' slots of static texels (so that the dense stack reads consistently: flush); static_tied != 0
 * tells the step that frame 0 of the gradient already holds a static texel's frame sum (vl3d_tie_static_grad ran on it).
 * mirror_static bit 1 ("lean" compact copy): the caller guarantees that `compact` holds FINITE values everywhere already (a persistent
 * buffer that was zero-filled once and has only ever been written by this call), so the slots the render cannot read with a non-zero
 * weight -- culled texels, texels outside their plane's box -- are not written: for a tile-culled model they were most of the copy. */
int32_t vl3d_adam_window_tile(void);
/* One argument for the whole family: the model, the window, the optimiser's state and hyper-parameters.  Which entry reads what:
 *   vl3d_adam_window_catchup  everything but lr / step and the two scratch pointers;
 *   vl3d_adam_window_step     everything but the two scratch pointers;
 *   vl3d_adam_flush_older     the model, the state, betas / eps, the quad maps and `blocks` -- not the window, not the boxes, not lr / step;
 *   vl3d_render_bwd_adam      everything (boxes_scratch / class_scratch are this entry's only).
 * Every entry refuses, before it launches anything, a struct whose dims are not positive (D <= 65535), whose window (where it is read) leaves the
 * plane or the bookkeeping tiles, `blocks` without quad maps, a quad grid of mixed signs or a tile-exact grid that does not divide the plane into
 * tiles of at least 2 x 2 texels, and a NULL state pointer.  The layout is ABI (152 bytes, `blocks` at 144: asserted in csrc/vl3d_optim.hip and
 * tests/test_adam_window_cpu.py). */
typedef struct vl3d_adam_window {
    int32_t D, T;                /* the model: param / exp_avg / exp_avg_sq are (D,T,Hs,Ws,4), or the pools of `blocks` */
    int32_t Hs, Ws;              /* the full planes */
    int32_t y0, x0, wh, ww;      /* the window [y0, y0 + wh) x [x0, x0 + ww), aligned to vl3d_adam_window_tile() or ending at the plane border */
    float *param, *exp_avg, *exp_avg_sq;
    int32_t *last_step;
    const float *hist;
    float lr, beta1, beta2, eps;
    int64_t step;
    /* Per-plane boxes, HOST [D][4] = (y0, y1, x0, x1) in plane texels, tile aligned, inside the window, or NULL: 16 bytes per plane that travel
     * in the kernel arguments, no copy, no synchronisation (NULL, or more than 128 planes: the whole window for every plane).  The window of a
     * crop is the union of the planes' footprints; texels of the window outside their own plane's box cannot be sampled in this iteration, their
     * gradient is exactly zero and their update stays deferred like that of every texel outside the window: the catch-up leaves their slots of the
     * compact copy unwritten (never read), the step skips them. */
    const int32_t *plane_boxes;
    void *boxes_scratch;         /* vl3d_render_bwd_adam: device, 16 * D bytes; required with plane_boxes */
    /* tile-culled model (NULL quad_keep: dense): the quad maps (device byte maps [D][|QH|][|QW|], a negative grid: tile-exact layout) and, for
     * vl3d_render_bwd_adam, a device scratch of vl3d_render_bwd_adam_class_bytes(desc) bytes for the texel records of the window (8 bytes per
     * plane texel: class, the step its bookkeeping tile is current for, its slot in the parameter tensors / pools -- written by the pre-pass,
     * read by the owner's store) */
    const uint8_t *quad_keep, *quad_dyn;
    int32_t QH, QW;
    void *class_scratch;
    const int32_t *blocks;       /* PACKED storage ("PACKED storage" below; needs the quad maps): param / exp_avg / exp_avg_sq are the pools */
} vl3d_adam_window;
int vl3d_adam_window_catchup(const vl3d_adam_window *w, int32_t upto, float *compact, float culled_alpha, int32_t mirror_static,
                             vl3d_stream_t stream);
int vl3d_adam_window_step(const vl3d_adam_window *w, const float *grad_compact, int32_t static_tied, vl3d_stream_t stream);
/* Bound on the deferral: every bookkeeping tile that has missed at least min_depth steps is replayed up to `upto`, written back and marked
 * (the others are left alone).  Run after each step it keeps what a returning crop window has to replay below min_depth steps per texel
 * -- the reference shuffles 32-72 crops x views per epoch (train_3dvid.py:263-290), so a window comes back after that many steps. */
int vl3d_adam_flush_older(const vl3d_adam_window *w, int32_t upto, int32_t min_depth, vl3d_stream_t stream);
void vl3d_adam_step_scalars(float lr, float beta1, float beta2, int64_t step, float *lr_bc1, float *bc2s);

/* The optimiser step INSIDE the render backward (train_3dvid.py:242-244: loss.backward(); optimizer.step() -- for the dense stage-2 model
 * they are one pass over the window's texels).  vl3d_render_bwd of the crop-aware iteration writes the window's compact gradient
 * (one stream) only for vl3d_adam_window_step to read it back beside (p, m, v) and write (p, m, v): 2 + 7 streams of the window.  Here the
 * owner-computes backward applies the step of `adam->step` where it would have stored a texel's complete gradient sum: 1 (taps) + 2 (m, v)
 * + 3 (p, m, v) streams, no gradient round trip.  `stack` is the compact copy of the texel window at (adam->y0, adam->x0) of the
 * (D,T,adam->Hs,adam->Ws,4) parameter -- desc->Hs x desc->Ws texels, written by vl3d_adam_window_catchup with upto = step - 1, so it
 * holds the parameters current for step - 1 and only the two moments are replayed (multiplications); adam->D, T, wh, ww must be
 * desc->D, T, Hs, Ws (VL3D_EINVAL otherwise).  Window / plane_boxes / last_step / hist: as vl3d_adam_window_step (hist[step] is written
 * by this call); on return the window's tiles are marked `step` and (p, m, v) are bit for bit what vl3d_render_bwd followed by vl3d_adam_window_step would have left (tests/test_gpu_optim.py).  Every texel of
 * window and box is stepped exactly once: by the tile that owns it, or -- texels no tile's gather reaches: zero gradient -- by the
 * backward's pre-pass.  grad_stack (the compact gradient, desc's dims) is still required: when the device-side plan finds the view
 * infeasible for the owner-computes kernels the atomics kernel fills it and the step kernel runs behind it, decided on the device (no
 * host synchronisation either way); it is left unwritten otherwise.
 * Tile-culled models (adam->quad_keep != NULL; the render culls with the same map, desc->cull_* = the window (y0, x0) of the (Hs, Ws) plane):
 * a DYNAMIC texel is stepped in the owner's store, a STATIC texel (one parameter for all frames) has its gradient stored to grad_stack as
 * vl3d_render_bwd with a quad map does and the step kernel behind the backward sums it over the frames -- static texels only, unless the plan was
 * infeasible --, culled texels are nobody's (grad_stack holds defined values in static texels only).  adam->blocks: packed storage.
 * fp32 stacks, the planar convention with the shipped activations ((affine, hardcut, post), sigmoid / sigmoid); dense models: T >= 2,
 * desc->variant 0 (the frame pairs; tile-culled models always take the one-frame tile kernel: 32-wide regions, variant 3 = 64-wide); anything else: VL3D_EUNSUPPORTED,
 * nothing launched. */
int64_t vl3d_render_bwd_adam_class_bytes(const vl3d_render_desc *desc);
int vl3d_render_bwd_adam(const vl3d_render_desc *desc, const void *stack, const float *homos, const float *rgb, const float *alpha,
                         const float *grad_rgb, const float *grad_alpha, const float *grad_reg, const void *reg_state,
                         const float *grad_alpha_sums, float *grad_stack, void *scratch, int64_t scratch_bytes,
                         const vl3d_adam_window *adam, vl3d_stream_t stream);

/* PACKED storage of a tile-culled model (vl3d_adam_window's `blocks` != NULL; quad maps required): the reference keeps a
 * static atlas (one frame), a dynamic atlas (T frames) and no storage for culled quads (MPI.py:364-436, MPV.py:235-288).  Here
 * param / exp_avg / exp_avg_sq are pools of 8 x 8-texel blocks (vl3d_adam_window_tile()): blocks [D][ceil(Hs/8)][ceil(Ws/8)] int32 = -1 for
 * a block no kept quad can read (not stored), else slot << 1 | dynamic, a slot being 64 texels (1 KiB); a static block owns one slot, a
 * dynamic block T consecutive ones (frame-major).  The compact window copy / gradient the render kernels work on stay dense, so the
 * kernels of the hot path are unchanged and the parameters after every step have the bits of the dense (D,T,Hs,Ws,4) model; the pool of
 * a model with 16 % of its quads kept is about a seventh of the dense stack (videoloop3d_amd/packed.py). */
/* Chosen frames of a PACKED model as a dense stack for an evaluation render (MPV.py:439 `atlas_dyn[ts]`): out (D,n,Hs,Ws,4); frames =
 * device int32 [n], each in [0,T); blocks without storage read (0, 0, 0, culled_alpha), static blocks their one copy in every frame. */
int vl3d_packed_unpack_frames(int32_t D, int32_t T, int32_t Hs, int32_t Ws, const int32_t *blocks, const float *pool, int32_t n,
                              const int32_t *frames, float culled_alpha, float *out, vl3d_stream_t stream);
/* The forward of MPV.py:351-454 reading the PACKED texture directly -- the reference renders a sparsified model from its static / dynamic
 * tile lists (MPV.py:389-449), never from a dense texture.  desc: D, T (frames of the model), Hs x Ws (texels of a plane), the H x W view,
 * pixel_center / sx / sy / ox / oy, activations; convention (VL3D_COORD_AFFINE, VL3D_BORDER_HARDCUT, VL3D_ACT_POST), fp32.  blocks / pool:
 * as above; frames = device int32 [n]; quad_keep [D][QH][QW] = the map the block table was built from (a sample in a culled quad is not
 * covered).  rgb (n,H,W,3), alpha (n,H,W): the bits of vl3d_render_fwd with the same map on the unpacked frames.  Forward only (evaluation renders):
 * training renders from the compact window copy of the crop-aware optimiser (vl3d_adam_window_catchup). */
int vl3d_render_fwd_packed(const vl3d_render_desc *desc, const int32_t *blocks, const float *pool, const int32_t *frames, int32_t n,
                           const float *homos, const uint8_t *quad_keep, int32_t QH, int32_t QW, float culled_alpha, float *rgb,
                           float *alpha, vl3d_stream_t stream);

/* Layer-space smoothness regularisers (MPV.py:517-531 rgb_smooth / a_smooth; MPI.py:608-622) WITHOUT the materialised [T,h,w,K,4]
 * layer tensor: sums[0..3] (device doubles, overwritten) = sum over frames, layer SLOTS and neighbouring pixel pairs of |L[p]-L[q]|
 * for (x-pairs, rgb), (y-pairs, rgb), (x-pairs, alpha), (y-pairs, alpha).  L is the reference's `mpi` tensor: slot k of a pixel holds
 * the warped+activated rgba of the k-th nearest plane that COVERS it (masked_scatter over the rasteriser's z-sorted pix_to_face,
 * MPV.py:386-392, 441-449; unused slots 0) -- equal to plane k only where both pixels of a pair are covered by the same planes.
 * reg_state: caller-owned device buffer of vl3d_render_reg_state_bytes(desc) bytes, written by these forwards (per-pixel coverage
 * masks and pair flags; per (plane, frame, pixel) the signs of the four differences its layer value takes part in) and read by
 * vl3d_render_bwd, which takes the gradient w.r.t. the four sums as grad_reg = device float[4] (NULL: no regulariser term;
 * non-NULL requires the reg_state of the matching forward).  At most 128 planes.
 * quad_keep NULL = a dense model (QH, QW are not read), else the quad map and grid of vl3d_render_fwd: a culled quad's layer value is 0
 * like any uncovered pixel's.  No cull_scratch: the regulariser kernels walk the map themselves. */
int64_t vl3d_render_reg_state_bytes(const vl3d_render_desc *desc);
int vl3d_render_reg_fwd(const vl3d_render_desc *desc, const void *stack, const float *homos, const uint8_t *quad_keep, int32_t QH, int32_t QW,
                        double *sums, void *reg_state, vl3d_stream_t stream);
/* vl3d_render_fwd and vl3d_render_reg_fwd in ONE pass over the stack: what MPMeshVid.forward needs per training step when rgb_smooth /
 * a_smooth are on (configs/mpv_base.txt:33-34).  rgb / alpha / alpha_sums bit-identical to vl3d_render_fwd, sums / reg_state as
 * vl3d_render_reg_fwd writes them.  quad_keep NULL = a dense model (QH, QW are not read), else the whole forward of a tile-culled model
 * from its quad map and grid: the slot kernel visits every covered plane of every pixel nearest first, which is the order of the
 * over-composite, so the render falls out of the samples it takes anyway. */
int vl3d_render_fwd_reg(const vl3d_render_desc *desc, const void *stack, const float *homos, const uint8_t *quad_keep, int32_t QH, int32_t QW,
                        float *rgb, float *alpha, float *alpha_sums, double *sums, void *reg_state, vl3d_stream_t stream);

/* Stage 1's learned loop mask (MPI.py:115-117 `atlas_mask`, 568-583) as a FIFTH composited channel of the same pass:
 *     label(pixel) = sum_k w_k sigmoid(sample(mask_k)),   w_k = a_k T_k  the colour composite's blend weights,
 * sampled with the colour taps' positions and weights (grid_sample over the same uvs, MPI.py:569-572), and the weights DETACHED
 * (MPI.py:577-579 "detach mpi so that geometry is not related to mpi"): grad_label reaches the mask texture only.
 *   mask (D,T,Hs,Ws) logits, one float per texel of the stack;  label (T,H,W);  grad_mask (D,T,Hs,Ws) overwritten.
 * vl3d_render_fwd_mask: sums / reg_state both NULL = vl3d_render_fwd plus the label, both given = vl3d_render_fwd_reg plus the label
 * (rgb, alpha, alpha_sums, sums, reg_state exactly as those write them).  vl3d_render_bwd_mask = vl3d_render_bwd plus grad_label ->
 * grad_mask in the same sweep and gather (one frame per thread; grad_stack as vl3d_render_bwd computes it).  Built for the planar
 * convention stage 1 ships -- (VL3D_COORD_AFFINE, VL3D_BORDER_HARDCUT, VL3D_ACT_POST), sigmoid / sigmoid, fp32 stack, no quad map
 * (the reference drops the mask when it sparsifies, MPI.py:440-441); any other descriptor returns VL3D_EUNSUPPORTED and the caller
 * renders the label in a pass of its own (a stack whose channel 0 is the mask logit and channel 3 the alpha logit). */
int vl3d_render_fwd_mask(const vl3d_render_desc *desc, const void *stack, const float *mask, const float *homos, float *rgb,
                         float *alpha, float *label, float *alpha_sums, double *sums, void *reg_state, vl3d_stream_t stream);
int vl3d_render_bwd_mask(const vl3d_render_desc *desc, const void *stack, const float *mask, const float *homos, const float *rgb,
                         const float *alpha, const float *grad_rgb, const float *grad_alpha, const float *grad_label,
                         const float *grad_reg, const void *reg_state, const float *grad_alpha_sums, float *grad_stack,
                         float *grad_mask, void *scratch, int64_t scratch_bytes, vl3d_stream_t stream);

/* ... and the label alone when add_uv_noise is on (MPI.py:519-522 with :568-583): the reference jitters the COLOUR samples' UVs but samples the loop
 * mask at the UNJITTERED UVs and composites sigmoid(mask) with the detached alphas of the jittered samples -- two sampling positions per layer,
 * which the fused label channel above does not have (it refuses desc->uv_noise_seed != 0).  label (T,H,W) = sum_k w_k sigmoid(sample(mask_k, uv)),
 * w_k = a_k T_k with a_k = alpha_act(sample(alpha_k, uv + jitter_k)) x coverage(uv): the alphas the colour pass of the SAME desc->uv_noise_seed
 * composites with (same counter-hash field).  Gradient to the mask texture only (grad_mask (D,T,Hs,Ws), overwritten).  Planar convention
 * (affine, hardcut, post), fp32 stack, any alpha activation.  A completeness path (no shipped configuration sets add_uv_noise): plain kernels. */
int vl3d_label_noise_fwd(const vl3d_render_desc *desc, const float *stack, const float *mask, const float *homos, float *label, vl3d_stream_t stream);
int vl3d_label_noise_bwd(const vl3d_render_desc *desc, const float *stack, const float *mask, const float *homos, const float *grad_label,
                         float *grad_mask, vl3d_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Unfused operators (drop-ins for the reference's L3 functions).
 *
 * vl3d_warp_*: utils_mpi.py:159-176 warp_homography(h, w, homos[N,3,3], images[N,C,Hs,Ws]) -> [N,C,h,w]
 * with N = B*D (bilinear, zeros padding, align_corners=True under the utils_mpi normalisation). */
int vl3d_warp_fwd(int32_t N, int32_t C, int32_t Hs, int32_t Ws, int32_t h, int32_t w,
                  const float *homos, const float *images, float *out, vl3d_stream_t stream);
int vl3d_warp_bwd(int32_t N, int32_t C, int32_t Hs, int32_t Ws, int32_t h, int32_t w,
                  const float *homos, const float *grad_out, float *grad_images, vl3d_stream_t stream);

/* vl3d_overcompose_*: utils_mpi.py:92-107 overcompose(alpha[P,D], content[P,D,C]) -> rgb[P,C], blendweight[P,D];
 * front = index 0; P = B*H*W pixels. */
int vl3d_overcompose_fwd(int64_t P, int32_t D, int32_t C, const float *alpha, const float *content,
                         float *rgb, float *blendweight, vl3d_stream_t stream);
/* grad_bw may be NULL. */
int vl3d_overcompose_bwd(int64_t P, int32_t D, int32_t C, const float *alpha, const float *content,
                         const float *grad_rgb, const float *grad_bw,
                         float *grad_alpha, float *grad_content, vl3d_stream_t stream);

/* vl3d_overcompose_nto0_*: utils_mpi.py:110-132 overcomposeNto0; front = LAST plane index.
 * alpha[b,d,hw] at alpha + b*a_sb + d*a_sd + hw ; content[b,d,c,hw] at content + b*c_sb + d*c_sd + c*c_sc + hw
 * (element strides, so slices of mpi[B,D,4,H,W] need no copy).  rgb [B,C,HW]; trans [B,D,HW] (the
 * transmittance the reference returns as `blendweight` when ret_mask=True; may be NULL). */
int vl3d_overcompose_nto0_fwd(int32_t B, int32_t D, int32_t C, int64_t HW,
                              const float *alpha, int64_t a_sb, int64_t a_sd,
                              const float *content, int64_t c_sb, int64_t c_sd, int64_t c_sc,
                              float *rgb, float *trans, vl3d_stream_t stream);
/* grad_alpha [B,D,HW], grad_content [B,D,C,HW] dense. */
int vl3d_overcompose_nto0_bwd(int32_t B, int32_t D, int32_t C, int64_t HW,
                              const float *alpha, int64_t a_sb, int64_t a_sd,
                              const float *content, int64_t c_sb, int64_t c_sd, int64_t c_sc,
                              const float *grad_rgb, float *grad_alpha, float *grad_content,
                              vl3d_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Looping loss (utils_vid.py).  x is [3,Tx,H,W], y is [3,Ty,H,W] (batch 1, already trimmed to the
 * patch grid: utils_vid.py:307-320); element strides are given per (channel, frame, row), columns
 * are unit-stride.  Patch grid: h_o=(H-ps)/stride+1, w_o=(W-ps)/stride+1, n1=(Tx-pt)/stridet+1,
 * n2=(Ty-pt)/stridet+1. */
typedef struct vl3d_loss_desc {
    int32_t Tx, Ty, H, W;
    int32_t ps, pt, stride, stridet;
    int32_t use_alpha;     /* 0: plain NN (alpha > 100 in the reference, utils_vid.py:208) */
    float alpha;           /* utils_vid.py:133-134 normaliser offset */
    int64_t x_sc, x_st, x_sr;
    int64_t y_sc, y_st, y_sr;
    int32_t variant;       /* kernel variant selector for A/B measurements and cross-checks; 0 = default.  Bits 0-3, vl3d_patchnn: 2 one location
                            * per workgroup (1, the removed strided-staging kernel's number, and every value not named here run it too), 4 the
                            * vector-ALU kernel, 6 the split-f16 matrix-core kernel, 0 the measured default among them -- the rules and their
                            * limits: choose_patchnn(), csrc/vl3d_patchnn_choice.h; ask vl3d_patchnn_choice(); vl3d_vote_fold: 1 = the unstaged
                            * kernel.  Bits 4-7: refused (ablation switches of a -DVL3D_VARIANTS measurement build).  Bit 8: see vl3d_patchnn.
                            * Bit 9 (0x200), staged fold: dynamic covering loops.  Bit 11 (0x800), kernel 6: the workgroup-wide epilogue also
                            * without alpha.  Bits 12-15, vl3d_vote_fold*: tile shape index + 1 (choose_fold(), same header). */
} vl3d_loss_desc;

/* bytes of device scratch vl3d_patchnn / vl3d_patchnn_prepared need for this problem: positive for every valid descriptor. */
int64_t vl3d_patchnn_scratch_bytes(const vl3d_loss_desc *desc);

/* Which kernel a search or a fold call runs, without running it: the value the entry points themselves compute (the same function, no
 * device touched, nothing enqueued).  They return what the entry would return for the descriptor and these facts: its descriptor check,
 * then the chooser's status (VL3D_EINVAL / VL3D_EUNSUPPORTED leave *out zeroed).  entry: which search entry; has_scratch: scratch != NULL;
 * x_pitch, x_frames: vl3d_patchnn_grams' x clip; y_pitch: the prepared y clip's (both unread at VL3D_NN_ENTRY_PLAIN).  fused: vl3d_vote_fold_robust*. */
enum { VL3D_NN_ENTRY_PLAIN = 0, VL3D_NN_ENTRY_PREPARED = 1, VL3D_NN_ENTRY_GRAMS = 2 };
enum { VL3D_NN_LAYOUT_GRAM16 = 1, VL3D_NN_LAYOUT_PIXEL_MAJOR = 2 };
typedef struct vl3d_nn_choice {
    int32_t kernel;                        /* 2, 4 or 6: the variant numbers */
    int32_t tyt, nl, nw, xs, ch;           /* kernel 6: patchnn6_k<tyt, nl, nw, xs>, columns per LDS-DMA stage */
    int32_t runsum;                        /* kernel 4: patchnn4_k<runsum, threads> */
    int32_t threads;                       /* workgroup size */
    int32_t kc;                            /* kernel 2: k terms staged at a time */
    int32_t lds_bytes;                     /* dynamic LDS of the launch */
    int32_t scratch_layout;                /* VL3D_NN_LAYOUT_*: the form of x and y the kernel reads (what `scratch` holds) */
} vl3d_nn_choice;
int vl3d_patchnn_choice(const vl3d_loss_desc *desc, int32_t entry, int32_t has_scratch, int32_t x_pitch, int32_t x_frames, int32_t y_pitch,
                        vl3d_nn_choice *out);
typedef struct vl3d_fold_choice {
    int32_t staged;                        /* the LDS-staged kernel (else one thread per voxel, vl3d_vote_fold only) */
    int32_t shape;                         /* staged: row of the tile-shape table, -1 otherwise */
    int32_t fw, fh, threads;               /* staged: vote_fold_lds_k<fw, fh, threads, nb> */
    int32_t nb;                            /* staged: fixed-trip covering loops over nb x nb locations (2, 3), 0 = dynamic loops */
    int32_t lds_bytes;
} vl3d_fold_choice;
int vl3d_vote_fold_choice(const vl3d_loss_desc *desc, int32_t fused, vl3d_fold_choice *out);

/* Per spatial location b=(by,bx): dist[i,j] = |Px_i - Py_j|^2 / (3*pt*ps*ps) (utils_vid.py:72-86),
 * optional column-min normalisation (utils_vid.py:109-119,133-134), row argmin, first minimum wins
 * (utils_vid.py:139-141).  nn is int32 [h_o, w_o, n1].  Replaces extract_3Dpatches x2 +
 * get_NN_indices_low_memory (utils_vid.py:209-216).
 * The kernel works on pixel-major copies of x and y kept in `scratch`, vl3d_patchnn_scratch_bytes(desc) bytes (their layout belongs to the
 * kernel variant: a scratch filled under one variant is not valid for another); scratch == NULL: VL3D_EINVAL -- the kernel that read the
 * videos in place was removed, and desc->variant 1, its number, runs kernel 2 like every value not named.  desc->variant bit 8 (0x100): the y copy in `scratch`
 * is still valid from the previous call with the same y, configuration and scratch buffer -- skip re-building it (the
 * captured video y is constant over the iterations of a training loop; x, the render, is not). */
int vl3d_patchnn(const vl3d_loss_desc *desc, const float *x, const float *y, int32_t *nn,
                 void *scratch, vl3d_stream_t stream);

/* The captured clip y is constant training data (train_3dvid.py:22-66 crops it per iteration, MPV.py:506 hands the crop to the loss):
 * vl3d_video_to_gram_major rewrites a whole clip [3,T,H,W] (element strides per channel / frame / row, unit column stride) ONCE into
 * the NN kernel's own form (vl3d_gram_major_bytes(T, H, W) bytes), and vl3d_patchnn_prepared searches against the crop
 * (y_row0, y_col0) + (desc->H, desc->W) of that buffer (rows of y_pitch pixels, y_rows of them; desc->Ty = T) without touching y again
 * -- the y half of the per-iteration layout change (0.4 of the 2.7 ms of a 720p search) leaves the iteration.  Matrix-core kernel only:
 * VL3D_EUNSUPPORTED outside its range (choose_patchnn(); vl3d_patchnn_choice() tells), and the caller falls back to vl3d_patchnn.  `scratch`
 * as for vl3d_patchnn. */
int64_t vl3d_gram_major_bytes(int32_t T, int32_t H, int32_t W);
int vl3d_video_to_gram_major(const float *y, int64_t sc, int64_t st, int64_t sr, int32_t T, int32_t H, int32_t W, float *out,
                             vl3d_stream_t stream);
int vl3d_patchnn_prepared(const vl3d_loss_desc *desc, const float *x, const float *y_gram, int32_t y_pitch, int32_t y_rows,
                          int32_t y_row0, int32_t y_col0, int32_t *nn, void *scratch, vl3d_stream_t stream);
/* ... with x in that form too (vl3d_loop_pad_fwd_gram writes it beside the video: the render's output is read once for both layouts of the
 * loss, MPV.py:484-507 -> utils_vid.py:209-216): x_gram holds an x_rows x x_pitch clip of x_frames frames, desc (Tx, H, W) names its
 * leading frames / rows / columns (the loss's trim to the patch grid, utils_vid.py:307-320).  No scratch. */
int vl3d_patchnn_grams(const vl3d_loss_desc *desc, const float *x_gram, int32_t x_pitch, int32_t x_rows, int32_t x_frames, const float *y_gram,
                       int32_t y_pitch, int32_t y_rows, int32_t y_row0, int32_t y_col0, int32_t *nn, vl3d_stream_t stream);

/* get_NN_indices_low_memory(X[B,n1,...], Y[B,n2,...], alpha, chunksz, 'mse') on MATERIALISED patches
 * (utils_vid.py:122-142; the caller evaluations/NNMSE.py:45-56 builds them with extract_3Dpatches).
 * X [B,n1,d], Y [B,n2,d] dense fp32; nn int64 [B,n1] like the reference's torch.long. */
int vl3d_nn_vectors(int64_t B, int32_t n1, int32_t n2, int32_t d, const float *X, const float *Y,
                    int32_t use_alpha, float alpha, int64_t *nn, vl3d_stream_t stream);

/* Gather the NN patches of y and vote-fold them onto x's grid (utils_vid.py:217-229):
 * sum [3,Tx,H,W] dense, weight [Tx,H,W] dense = vote count clamped at 1e-10.
 * normalize != 0 writes sum/weight (utils_vid.py:344) instead of the raw sum. */
int vl3d_vote_fold(const vl3d_loss_desc *desc, const float *y, const int32_t *nn,
                   float *sum, float *weight, int32_t normalize, vl3d_stream_t stream);

/* NN-error metric support (evaluations/NNMSE.py:45-56): err[h_o*w_o] (overwritten) = per patch location the sum over its
 * n1 patches and their 3*pt*ps*ps elements of |y patch at nn - x patch|; nn from vl3d_patchnn (use_alpha = 0). */
int vl3d_patch_l1(const vl3d_loss_desc *desc, const float *x, const float *y, const int32_t *nn, float *err,
                  vl3d_stream_t stream);

/* Fused vote-fold + robust loss (utils_vid.py:217-229 + :344 + :348 in one pass): y2x = fold(y, nn) / weight is written
 * (the loss classes cache it as last_y2x), and while it is in a register the robust loss of (x - y2x) is summed into
 * loss_sum (device double, overwritten) and grad_x (3,Tx,H,W contiguous) receives d mean(rho)/dx = rho'(x - y2x) / (3 Tx H W).
 * x uses the strides of desc.  Replaces vl3d_vote_fold(normalize=1) + vl3d_robust_fwd + vl3d_robust_bwd. */
int vl3d_vote_fold_robust(const vl3d_loss_desc *desc, const float *y, const int32_t *nn, const float *x, int32_t rho_kind,
                          float rou, float scale, float *y2x, float *weight, float *grad_x, double *loss_sum,
                          vl3d_stream_t stream);

/* The same with grad_x addressed through strides (elements): channel, frame, row; unit column stride.  The reference trims x to the
 * patch grid by slicing before the loss (utils_vid.py:307-320), so the gradient of the untrimmed x is zero outside the trimmed box:
 * the caller hands a zero-filled buffer of x's FULL shape and its strides, and the slice's backward (a zero fill and a copy per sliced
 * axis) never runs. */
/* y2x and weight may both be NULL: the vote average then stays in registers (767 MB of stores less per 720p iteration; the loss
 * classes materialise last_y2x / last_weight on first access through vl3d_vote_fold). */
int vl3d_vote_fold_robust_strided(const vl3d_loss_desc *desc, const float *y, const int32_t *nn, const float *x, int32_t rho_kind,
                                  float rou, float scale, float *y2x, float *weight, float *grad_x, int64_t gx_sc, int64_t gx_st,
                                  int64_t gx_sr, double *loss_sum, vl3d_stream_t stream);

/* x[0..n) *= *scale with `scale` a DEVICE scalar (no host sync); no memory traffic at all when it is exactly 1 -- the backward of the fused
 * looping loss: its gradient buffer exists since the forward and the upstream gradient of a loss differentiated directly is 1.  n % 4 == 0. */
int vl3d_scale_inplace(int64_t n, float *x, const float *scale, vl3d_stream_t stream);

/* The loss prologue of MPMeshVid.forward (MPV.py:484-507), from the render's NHWC output to the loss's video in three launches:
 *   rgb_pad = cat(rgb, rgb[:pad])                                       loop padding (MPV.py:490-492)
 *   scale   = (exp(mean(log((mean_f res + 0.01) / (mean_t rgb + 0.01)))) + 3) / 4     scale-invariant gain (MPV.py:499-504; rgb detached)
 *   x       = rgb_pad * scale,  handed to the loss as [1,3,T+pad,h,w]
 * vl3d_loop_gain: rgb (T,h,w,3), res (F,3,h,w) -> *log_sum (device double, zeroed by the call) = the sum of the 3 h w log ratios.
 * vl3d_loop_pad_fwd: x (3,T+pad,h,w) = gain * rgb with the first `pad` frames repeated at the end; log_sum == NULL: gain 1.
 * vl3d_loop_pad_bwd: grad_rgb (T,h,w,3) = gain * (grad_x[:, t] + grad_x[:, T + t] for t < pad); grad_x (3,T+pad,h,w) with channel /
 * frame strides gx_sc / gx_st in floats (unit column stride, rows contiguous). */
int vl3d_loop_gain(int32_t T, int32_t F, int32_t h, int32_t w, const float *rgb, const float *res, double *log_sum, vl3d_stream_t stream);
/* ... with res (F,3,h,w) read through strides in floats (r_sf frame, r_sc channel, r_sr row; unit column stride): a crop of the captured clip as it lies. */
int vl3d_loop_gain_strided(int32_t T, int32_t F, int32_t h, int32_t w, const float *rgb, const float *res, int64_t r_sf, int64_t r_sc, int64_t r_sr,
                           double *log_sum, vl3d_stream_t stream);
int vl3d_loop_pad_fwd(int32_t T, int32_t pad, int32_t h, int32_t w, const float *rgb, const double *log_sum, float *x, vl3d_stream_t stream);
/* ... writing, beside x, its form for the NN search: x_gram = vl3d_gram_major_bytes(T + pad, h, w) bytes (for vl3d_patchnn_grams). */
int vl3d_loop_pad_fwd_gram(int32_t T, int32_t pad, int32_t h, int32_t w, const float *rgb, const double *log_sum, float *x, float *x_gram,
                           vl3d_stream_t stream);
int vl3d_loop_pad_bwd(int32_t T, int32_t pad, int32_t h, int32_t w, const float *grad_x, int64_t gx_sc, int64_t gx_st, const double *log_sum,
                      float *grad_rgb, vl3d_stream_t stream);

/* Per-pixel terms of MPMesh.forward / MPMeshVid.forward after the fused render, one pass each way instead of ~30 scalar launches:
 *   sums[0] = sum_p  n1_p / max(sqrt(max(n2_p, 1e-30)), eps)      sparsity (MPI.py:599-603, MPV.py:511-515), (n1, n2) = alpha_sums (n,2) = (sum_k a_k, sum_k a_k^2)
 *   sums[1] = sum_p | alpha_p - 1 |                               density  (MPI.py:647-650, MPV.py:533-536)
 * either input may be NULL (its sum stays 0).  grad_alpha_sums (n,2) / grad_alpha (n), optional: d sums[0] / d alpha_sums, d sums[1] / d alpha
 * (unit upstream gradient, not divided by n: the caller scales).  sums: device double[2], overwritten. */
int vl3d_pixel_terms(int64_t n, const float *alpha, const float *alpha_sums, float eps, double *sums, float *grad_alpha_sums, float *grad_alpha,
                     vl3d_stream_t stream);

/* Stage 1's image + loop-mask loss (train_3d.py:200-220) on the module's output rgbl (B,C,h,w), C = 3 | 4, read through strides in floats
 * (sb batch, sc channel, sp pixel: the NHWC render output viewed as NCHW); target (B,3,h,w), target_mask (B,h,w) contiguous:
 *   s       = scale_invariant ? (exp(mean log((target + .01) / (rgb + .01))) + 3) / 4 : 1          (rgb detached in it, as in the reference)
 *   sums[0] = sum (rgb s - target)^2                                     -> img_loss  = sums[0] / (3 B h w)
 *   sums[1] = - sum (m log l + (1 - m) log(1 - l)), l = clamp(label, .001, .999)     -> loop_loss = sums[1] / (B h w)      (C == 4)
 * grad (B,h,w,C) contiguous: d sums[0] / d rgb in channels 0-2, d sums[1] / d label in channel 3 (the caller divides by the counts and
 * multiplies by the upstream gradients).  log_sum: device double scratch; sums: device double[2]; both overwritten. */
int vl3d_stage1_loss(int32_t B, int32_t C, int32_t h, int32_t w, const float *rgbl, int64_t sb, int64_t sc, int64_t sp, const float *target,
                     const float *target_mask, int32_t scale_invariant, double *log_sum, double *sums, float *grad, vl3d_stream_t stream);

/* The whole scalar head of a stage-1 iteration (train_3d.py:200-232 on MPI.py:596-652's outputs) in one sweep over the crop's pixels:
 *   img_loss, loop_loss as vl3d_stage1_loss; sparsity, density as vl3d_pixel_terms (sparsity times `sparsity_scale` = 1 / sqrt(mpi_d));
 *   rgb_smooth = coef0 s0 + coef1 s1, a_smooth = coef2 s2 + coef3 s3 from the render's four smoothness sums (MPI.py:605-619);
 *   total = w_img img + w_loop loop + w_sparsity sparsity + w_density density + w_rgb_smooth rgb_smooth + w_a_smooth a_smooth.
 * Inputs are the render's own outputs: rgb (B,h,w,3), label (B,h,w) | NULL, alpha (B,h,w) | NULL, alpha_sums (B,h,w,2) | NULL,
 * smooth_sums float[4] | NULL; target (B,3,h,w) and target_mask (B,h,w) | NULL (with label) through strides in floats (t_sb batch, t_sc channel,
 * t_sr row; m_sb, m_sr; unit column stride: a crop of a larger image needs no copy).  Outputs: out float[8] = (total, img, loop,
 * w sparsity, w density, w rgb_smooth, w a_smooth, gain) and the gradients of `total` w.r.t. every given input, FINAL for a unit upstream
 * gradient (the caller scales them by the actual one: vl3d_scale_inplace skips the pass when it is 1).  scratch: 6 device doubles. */
typedef struct vl3d_stage1_objective_desc {
    int32_t B, h, w;
    int32_t scale_invariant;
    float w_img, w_loop, w_sparsity, w_density, w_rgb_smooth, w_a_smooth;
    float sparsity_scale, eps;
    float smooth_coef[4];
} vl3d_stage1_objective_desc;
int vl3d_stage1_objective(const vl3d_stage1_objective_desc *desc, const float *rgb, const float *label, const float *alpha, const float *alpha_sums,
                          const float *smooth_sums, const float *target, int64_t t_sb, int64_t t_sc, int64_t t_sr, const float *target_mask,
                          int64_t m_sb, int64_t m_sr, double *scratch, float *out, float *grad_rgb,
                          float *grad_label, float *grad_alpha, float *grad_alpha_sums, float *grad_smooth, vl3d_stream_t stream);

/* The weighted total of a stage-2 iteration (train_3dvid.py:230-240: loss = swd + sum_k weight_k term_k) over n <= 16 device scalars
 * v = (*main_term, rest[0..n-2]) with device coefficients coef[n]; term i belongs to group (groups >> 4 i) & 15 of `ngroups` <= 16 (a smoothness
 * mean is two of the render's four sums): out[0] = sum_i coef_i v_i, out[1 + g] = the sum of group g's terms (one launch instead of a stack, a
 * multiply and a sum on one-element tensors and their autograd mirrors).  Backward: grad_terms[i] = coef_i * *grad_total. */
int vl3d_linear_head_fwd(int32_t n, uint64_t groups, int32_t ngroups, const float *main_term, const float *rest, const float *coef, float *out,
                         vl3d_stream_t stream);
int vl3d_linear_head_bwd(int32_t n, const float *coef, const float *grad_total, float *grad_terms, vl3d_stream_t stream);

/* robust_lossfun (utils_vid.py:10-26) fused with the mean (utils_vid.py:348).
 * kind: 0 'mse', 1 'abs', 2 general Barron with float rou (rou==0 and rou==2 special-cased as the reference).
 * loss_sum: device double, overwritten with sum over n elements of rho(x - y2x). */
enum { VL3D_RHO_MSE = 0, VL3D_RHO_ABS = 1, VL3D_RHO_BARRON = 2 };
int vl3d_robust_fwd(int64_t n, const float *x, const float *y2x, int32_t kind, float rou, float scale,
                    double *loss_sum, vl3d_stream_t stream);
/* grad_x[i] = rho'(x[i]-y2x[i]) * (*grad_out) * inv_n ; grad_out is a DEVICE scalar (no host sync). */
int vl3d_robust_bwd(int64_t n, const float *x, const float *y2x, int32_t kind, float rou, float scale,
                    const float *grad_out, float inv_n, float *grad_x, vl3d_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Evaluation (scripts/script_evaluate_ours.py:149-181, evaluations/metrics.py:15-89 with skimage's structural_similarity /
 * peak_signal_noise_ratio as that file calls them).  One test view: gt uint8 [F,H0,W0,3] and pred uint8 [T,H0,W0,3] (F != T allowed),
 * each addressed through byte strides per frame (*_sf) and row (*_sr) with pixel stride 3 and channel stride 1; the crop window
 * (row0, col0, h, w) is read in place.  mask: uint8 [h,w] holding 0/1 (the static region, metrics.py:43-56), or NULL = all ones;
 * mask_ones = its number of ones, counted by the caller (1 .. h*w; an all-zero mask is refused with VL3D_EINVAL, where the reference
 * yields nan / -inf).  A sample is a = w / 255 with the integer w = (2u - 255) m.
 * Outputs, for every frame f < Fm = min(F, T):
 *   sse[f]      = sum over h*w*3 of (w_gt - w_pred)^2                       (int64, exact; mse = sse / (255^2 h w 3))
 *   ssim_sum[f] = sum over pixels and channels of S * m                      (fp64; frame SSIM = ssim_sum / sum(m) / 3, metrics.py:80)
 *                 S: skimage's SSIM map, win 7, uniform weights, data_range 2, cov_norm 49/48, window sums of scipy's uniform_filter
 *                 with mode 'reflect' (half-sample symmetric: d c b a | a b c d); the window sums are exact integers
 *   gt_min[f]   = min over h*w*3 of w_gt                                     (int32; skimage's data_range is 2 if < 0, else 1)
 * and dyn_sum[0] = sum over h*w*3 of (std_F(gt) - std_T(pred))^2 on 0..255 values, population std, each clip over its own frames
 * (script_evaluate_ours.py:176-178; dyn = dyn_sum / (h w 3)).  F, T <= 32768; h, w >= 7 (skimage's win_size; VL3D_EINVAL otherwise).
 * Two launches (statistics, then a fixed-order reduction over workgroups): no float atomics, identical bits on every call.
 * scratch: vl3d_eval_scratch_bytes(desc) bytes of device memory (-1 for an invalid descriptor). */
typedef struct vl3d_eval_desc {
    int32_t F, T;                  /* frames of gt / pred */
    int32_t row0, col0, h, w;      /* crop window */
    int64_t gt_sf, gt_sr;          /* byte strides of gt: frame, row */
    int64_t pred_sf, pred_sr;      /* byte strides of pred: frame, row */
} vl3d_eval_desc;
int64_t vl3d_eval_scratch_bytes(const vl3d_eval_desc *desc);
int vl3d_eval_view(const vl3d_eval_desc *desc, const uint8_t *gt, const uint8_t *pred, const uint8_t *mask, int64_t mask_ones,
                   int64_t *sse, double *ssim_sum, int32_t *gt_min, double *dyn_sum, void *scratch, vl3d_stream_t stream);

/* ---- Video I/O: 8-bit RGB frames <-> planar Y'CbCr as a YUV4MPEG2 payload holds it (docs/kernels/K10_video_io.md) ------------------------
 * The reference reads and writes its clips through cv2 / imageio (dataloader.py, script_render_video.py:149); this project has neither and
 * moves frames as .y4m files (videoloop3d_amd/y4m.py), whose only arithmetic is this conversion.  THE RULE is stated once, in integers, by
 * y4m.rgb8_to_yuv8 / y4m.yuv8_to_rgb8; both entries store its bytes, byte for byte, on either path:
 *   encode   byte = clamp((c0 R + c1 G + c2 B + offset 2^16 + 2^15) >> 16, 0, 255) with the integer rows of vl3d_video_coefs; 4:2:0 chroma
 *            takes the SUMS of the 2 x 2 block (coordinates clamped at the right / bottom edge of an odd frame) and shifts by 18; chroma
 *            planes are ceil(H/2) x ceil(W/2), centre sited.  The fourth channel of RGBA frames is not read.
 *   decode   chroma upsampled bilinearly as 16 x chroma with clamped indices: per axis weights (3, 1) / 4 on the own sample and the
 *            neighbour on the side of the luma coordinate's parity; siting_x LEFT horizontally (4, 0) / 4 on even and (2, 2) / 4 on odd
 *            columns; 4:4:4: 16 c.  byte = clamp((cy (Y - y0) + cu (U16 - 2048) + cv (V16 - 2048) + 2^20) >> 21, 0, 255), int32 throughout.
 *            Sink U8: uint8 [N,H,W,channels], a fourth channel is 255.  Sink F32: float [N,3,H,W] = byte / 255 (IEEE division).
 * Frames: frame n of plane p starts at p + n * frame_stride; rows are tight (W bytes of luma, cw of chroma); the RGB side is dense.
 * Two paths, the same bytes: WIDE -- a thread owns 16 luma pixels of 2 rows (1 row at 4:4:4) and moves them in 16- and 8-byte accesses,
 * taken when W is a multiple of 16, H even (4:2:0), and every pointer and the stride are aligned for it; BYTE -- everything else, one
 * byte per access.  desc->path = 1 forces the byte path; vl3d_video_choice tells which one a call takes (pure: nothing is launched).
 * VL3D_EINVAL, nothing launched: a NULL descriptor, plane or frame pointer; channels outside {3, 4} (F32 sink: 3); N, H or W < 1; an unknown
 * chroma, siting_x, matrix, full_range, sink or path; frame_stride below the frame's H W + 2 ch cw bytes; N H W above 2^31 - 1 (the grid
 * limit); an F32 sink that is not 4-byte aligned. */
enum { VL3D_CHROMA_444 = 0, VL3D_CHROMA_420 = 1 };
enum { VL3D_SITING_CENTER = 0, VL3D_SITING_LEFT = 1 };      /* horizontal siting read by the decode (C420jpeg / C420mpeg2); the encode is centre sited */
enum { VL3D_MATRIX_BT601 = 0, VL3D_MATRIX_BT709 = 1 };
enum { VL3D_SINK_U8 = 0, VL3D_SINK_F32 = 1 };
enum { VL3D_VIDEO_PATH_AUTO = 0, VL3D_VIDEO_PATH_BYTE = 1 };
typedef struct vl3d_video_desc {
    int32_t N, H, W, channels;                       /* frames, luma size, channels of the RGB side (3 / 4) */
    int32_t chroma, siting_x, matrix, full_range;    /* VL3D_CHROMA_*, VL3D_SITING_* (decode only), VL3D_MATRIX_*, 0 limited / 1 full */
    int32_t sink, path;                              /* decode: VL3D_SINK_*; VL3D_VIDEO_PATH_* */
    uint8_t *y, *u, *v;                              /* frame 0 of each plane (read by the decode, written by the encode) */
    int64_t frame_stride;                            /* bytes from a frame of a plane to the next, the same for all three */
} vl3d_video_desc;
typedef struct vl3d_video_path {
    int32_t wide;                                    /* 1: the wide path, 0: the byte path */
    int32_t strip, rows;                             /* luma pixels a thread owns: strip columns x rows */
    int32_t threads, blocks;                         /* the launch: workgroup size, workgroups */
} vl3d_video_path;
/* The rule's integers for (matrix, full_range), as the kernels use them -- enc[12]: the 3 x 3 rows at 2^16 (Y, U, V), then the three offsets;
 * dec[10]: per output channel (cy at 2^21, cu, cv at 2^17), then y0.  Pure host code. */
int vl3d_video_coefs(int32_t matrix, int32_t full_range, int32_t *enc, int32_t *dec);
/* rgb: the dense RGB side of the call (read by the encode, written by the decode); decode: 0 vl3d_rgb8_to_yuv8, 1 vl3d_yuv8_to_rgb. */
int vl3d_video_choice(const vl3d_video_desc *desc, const void *rgb, int32_t decode, vl3d_video_path *out);
int vl3d_rgb8_to_yuv8(const vl3d_video_desc *desc, const uint8_t *rgb, vl3d_stream_t stream);
int vl3d_yuv8_to_rgb(const vl3d_video_desc *desc, void *rgb, vl3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VL3D_H */
