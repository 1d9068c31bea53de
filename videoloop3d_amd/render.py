"""Fused differentiable MPI/MPV render (warp + sample + activate + composite) on the HIP kernels.

Host-side mirror of the chain MPV.py:351-454 (planar geometry) / utils_mpi.py:159-176 + 92-107 of the
reference, behind a torch.autograd.Function.  The arithmetic lives in csrc/vl3d_render.hip.
"""
import math
import types
from dataclasses import dataclass

import torch

from . import _lib as L


@dataclass(frozen=True)
class RenderSpec:
    """Sampling / compositing conventions (see oracle/mpi_oracle.py:RenderSpec for the CPU statement).

    Defaults = the utils_mpi convention (sigmoid -> warp_homography -> over-composite).
    `RenderSpec.mpv()` = the planar MPV.py convention (pixel centres at +0.5, hard-cut quad borders,
    sample-then-activate).  `act_order="baked"` (with the planar convention, sigmoid / sigmoid): the picture the viewer package shows --
    every tap activated, truncated to the byte baked.bake_texels writes, decoded, then blended (include/vl3d.h VL3D_ACT_BAKED); the gradient
    is the activate-first one, the rounding straight-through."""
    pixel_center: float = 0.0
    coord_mode: str = "utils_mpi"
    scale: tuple = (1.0, 1.0)
    offset: tuple = (0.0, 0.0)
    border: str = "zeros"
    act_order: str = "pre"
    rgb_act: str = "sigmoid"
    alpha_act: str = "sigmoid"
    variant: int = 0
    uv_noise_seed: int = 0      # add_uv_noise (MPV.py:420-423, MPI.py:519-522; include/vl3d.h): 0 = off, else the seed of this call's half-texel jitter field
    # TILE-EXACT layout of a tile-culled model (include/vl3d.h "Tile-exact layout"; needs quad_keep): (th, tw) texels per quad, every quad owning
    # its border row / column as the reference's sparsified atlases store them (MPI.py:380-418).  The planes are QH th x QW tw texels; `scale`
    # / `offset` then give the LATTICE coordinate (a quad spans tw - 1 of them) and the kernels add the quad index.  (0, 0): shared borders.
    tile: tuple = (0, 0)

    @staticmethod
    def mpv(rgb_act="sigmoid", alpha_act="sigmoid", scale=(1.0, 1.0), offset=(0.0, 0.0), variant=0):
        return RenderSpec(pixel_center=0.5, coord_mode="affine", scale=scale, offset=offset, border="hardcut",
                          act_order="post", rgb_act=rgb_act, alpha_act=alpha_act, variant=variant)


def _qgrid(quad_keep, spec):
    """(QH, QW) of a quad map as the C ABI takes them: negative for the tile-exact layout."""
    QH, QW = int(quad_keep.shape[1]), int(quad_keep.shape[2])
    return (-QH, -QW) if getattr(spec, "tile", (0, 0))[0] else (QH, QW)


def _qmap(quad_keep, spec):
    """(map, QH, QW) as every entry with a quad map takes them: (None, 0, 0) for a dense model."""
    return (None, 0, 0) if quad_keep is None else (L.ptr(quad_keep),) + _qgrid(quad_keep, spec)


def _desc_dims(D, T, Hs, Ws, H, W, spec, stack_dtype=0, row0=0, col0=0):
    """the render descriptor of `spec` for a model given by its dimensions (a stack, or the block table of a packed model)."""
    d = L.RenderDesc()
    d.D, d.T, d.Hs, d.Ws, d.H, d.W = int(D), int(T), int(Hs), int(Ws), int(H), int(W)
    d.row0, d.col0 = int(row0), int(col0)
    d.coord_mode = L.COORD[spec.coord_mode]
    d.border_mode = L.BORDER[spec.border]
    d.act_order = L.ACT_ORDER[spec.act_order]
    d.rgb_act, d.alpha_act = L.ACT[spec.rgb_act], L.ACT[spec.alpha_act]
    d.stack_dtype = int(stack_dtype)
    d.pixel_center = float(spec.pixel_center)
    d.sx, d.sy = float(spec.scale[0]), float(spec.scale[1])
    d.ox, d.oy = float(spec.offset[0]), float(spec.offset[1])
    d.variant = int(spec.variant)
    d.uv_noise_seed = int(getattr(spec, "uv_noise_seed", 0)) & 0xFFFFFFFF
    return d


def _desc(stack, H, W, spec, row0, col0, cull_window=None, grad_flags=0):
    D, T, Hs, Ws, C4 = stack.shape
    assert C4 == 4, "plane stack must be (D,T,Hs,Ws,4)"
    d = _desc_dims(D, T, Hs, Ws, H, W, spec, 1 if stack.dtype == torch.float16 else 0, row0, col0)
    if cull_window is not None:        # the stack is the texel window (y0, x0) of a (Hs_plane, Ws_plane) plane the quad grid lies over
        d.cull_row0, d.cull_col0, d.cull_Hs, d.cull_Ws = (int(v) for v in cull_window)
    d.grad_flags = int(grad_flags)
    return d


def _out_buffers(out, n, H, W, device, who):
    """(rgb [n,H,W,3], alpha [n,H,W]) float32: fresh, or the caller's `out` pair checked."""
    if out is None:
        return (torch.empty((n, H, W, 3), dtype=torch.float32, device=device), torch.empty((n, H, W), dtype=torch.float32, device=device))
    rgb, alpha = out
    if tuple(rgb.shape) != (n, H, W, 3) or tuple(alpha.shape) != (n, H, W) or not rgb.is_contiguous() or not alpha.is_contiguous():
        raise RuntimeError(f"{who}: `out` must be contiguous float32 (rgb [n,H,W,3], alpha [n,H,W])")
    return rgb, alpha


def _display_out(out, frames8, bg, n, H, W, device, who):
    """the display sink of a baked render (vl3d_baked_out.frames): `frames8` uint8 [n,H,W,3|4] contiguous on `device`, `bg` a sequence of 3
    floats or None -> (channels, bg as a host float[3] or None).  `out=` (the float sink) with `frames8=` is a ValueError; alignment of RGBA8
    frames and a non-finite background are the entry's refusals."""
    if out is not None:
        raise ValueError(f"{who}: `out=` (float32 rgb / alpha) and `frames8=` (uint8 display frames) name two different outputs: pass one")
    if not isinstance(frames8, torch.Tensor) or not frames8.is_cuda or frames8.device != device:
        raise RuntimeError(f"{who}: `frames8` must be a tensor on the model's device")
    if (frames8.dtype != torch.uint8 or frames8.dim() != 4 or tuple(frames8.shape[:3]) != (n, H, W) or frames8.shape[3] not in (3, 4)
            or not frames8.is_contiguous()):
        raise RuntimeError(f"{who}: `frames8` must be contiguous uint8 [n,H,W,3] (RGB8) or [n,H,W,4] (RGBA8) = [{n},{H},{W},3|4], "
                           f"got {tuple(frames8.shape)} {frames8.dtype}")
    if bg is not None:
        bg = [float(v) for v in bg]
        if len(bg) != 3:
            raise RuntimeError(f"{who}: `bg` is a colour of 3 floats, got {len(bg)}")
        bg = (L.C.c_float * 3)(*bg)
    return int(frames8.shape[3]), bg


def _quad_map(quad_keep, D):
    """the quad map [D,QH,QW] of a tile-culled model as the uint8 tensor the ABI reads."""
    L.check_cuda(quad_keep)
    if quad_keep.dim() != 3 or quad_keep.shape[0] != D:
        raise RuntimeError(f"quad_keep must be [D,QH,QW] with D = {D}, got {tuple(quad_keep.shape)}")
    from .tiles import as_u8
    return as_u8(quad_keep)


def _cull_scratch(desc, device):
    """the plane masks of a culled forward (vl3d_render_cull_scratch_bytes); call under torch.cuda.device(device)."""
    return torch.empty((int(L.lib().vl3d_render_cull_scratch_bytes(desc)) + 3) // 4, dtype=torch.float32, device=device)


# scratch (plan) buffer of the most recent backward: element 0 viewed as int32 is 1 when the LDS-staged
# owner-computes kernel ran, 0 when the call fell back to the atomics kernel (read by tests / diagnostics only).
LAST_BWD_SCRATCH = None
# ... and that backward's call as bwd_choice() takes it: (desc, entry, quad_keep, reg_grads, scratch_bytes); None after a backward
# vl3d_render_bwd_choice does not describe (the plane-rows band)
LAST_BWD_CALL = None


def bwd_choice(desc, entry="render", quad_keep=False, reg_grads=False, scratch_bytes=None):
    """which kernel a backward call with these arguments runs (vl3d_render_bwd_choice: the entry points' own decision, no device touched) ->
    L.BwdChoice.  scratch_bytes: None = what the wrappers pass (vl3d_render_bwd_scratch_bytes), 0 = no scratch."""
    out = L.BwdChoice()
    if scratch_bytes is None:
        scratch_bytes = int(L.lib().vl3d_render_bwd_scratch_bytes(desc))
    L.check(L.lib().vl3d_render_bwd_choice(desc, L.BWD_ENTRY[entry], int(bool(quad_keep)), int(bool(reg_grads)), int(scratch_bytes),
                                           int(entry == "adam"), L.C.byref(out)), "vl3d_render_bwd_choice")
    return out


def last_bwd_choice():
    """the choice of the most recent backward, as (family, width, rows, reg, mask, adam, cull, f16) with the family by name (L.BWD_FAMILY)."""
    if LAST_BWD_CALL is None:
        raise RuntimeError("last_bwd_choice(): no render backward has run yet, or the last one was a plane-rows band (its own frame-pair launch)")
    c = bwd_choice(*LAST_BWD_CALL)
    family = {v: k for k, v in L.BWD_FAMILY.items()}[c.family]
    return (family, c.width, c.rows) + tuple(bool(getattr(c, n)) for n in ("reg", "mask", "adam", "cull", "f16"))


class _RenderPlanes(torch.autograd.Function):
    @staticmethod
    def forward(ctx, stack, homos, H, W, spec, row0, col0, with_reg, quad_keep=None, cull_window=None, grad_culled_unwritten=False, fused_adam=None):
        ctx.set_materialize_grads(False)      # outputs the loss does not use come back as None, not as zero-filled tensors (a fill each, and reads in the backward kernels)
        L.check_cuda(stack, homos)
        # fused_adam (optim.WindowAdam with fused_backward): `stack` is its pending window leaf and the backward takes the step itself
        # (a tile-culled model: the optimiser classifies texels with ITS quad maps, the render culls with `quad_keep`: the same map, same device)
        ctx.fused_adam = fused_adam if (fused_adam is not None and (row0, col0) == (0, 0) and stack.is_contiguous()
                                        and (quad_keep is None) == (fused_adam.quad_keep is None)
                                        and (quad_keep is None or (cull_window is not None and tuple(quad_keep.shape) == tuple(fused_adam.quad_keep.shape)))
                                        and fused_adam.fuses(stack, spec)) else None
        ctx.leaf = stack if ctx.fused_adam is not None else None
        if quad_keep is not None:
            quad_keep = _quad_map(quad_keep, stack.shape[0])
        if stack.dtype not in (torch.float32, torch.float16):
            raise RuntimeError("plane stack must be float32 or float16 (arithmetic is fp32 either way)")
        if getattr(spec, "tile", (0, 0))[0] and quad_keep is None:
            raise RuntimeError("RenderSpec.tile (tile-exact layout) belongs to a tile-culled model: pass its quad_keep map")
        stack = stack.contiguous()
        # the camera gradient (vl3d_render_bwd_homos): only when `homos` asks for one -- otherwise nothing below changes, launch for launch
        ctx.cam = bool(ctx.needs_input_grad[1])
        if ctx.cam:
            _check_camera_grad(stack, spec, with_reg, fused_adam, quad_keep, cull_window)
            ctx.homos_like = (homos.dtype, homos.device)
        homos = homos.detach().to(torch.float32).contiguous()
        D, T = stack.shape[:2]
        if spec.coord_mode == "affine_planes":
            if homos.shape != (D, 16):
                raise RuntimeError(f"coord_mode 'affine_planes' takes per-plane records [D,16] = [{D},16] (atlas.plane_records), got {tuple(homos.shape)}")
            if quad_keep is not None:
                raise RuntimeError("tile culling is not available with per-plane texel transforms")
        elif homos.shape != (D, 3, 3):
            raise RuntimeError(f"homos must be [D,3,3] = [{D},3,3], got {tuple(homos.shape)}")
        rgb, alpha = _out_buffers(None, T, H, W, stack.device, "render_planes")
        ctx.nothing_to_render = T == 0 or H == 0 or W == 0
        if ctx.nothing_to_render:
            # an empty `ts` / zero-area crop: grid_sample + cumprod of the reference return empty tensors (MPV.py:425-454); the
            # ABI refuses non-positive dims, so the empty case never reaches it
            ctx.save_for_backward(stack)
            z = torch.zeros
            return (rgb, alpha, z(4, dtype=torch.float32, device=stack.device),
                    z((T, H, W, 2) if with_reg else (0,), dtype=torch.float32, device=stack.device))
        desc = _desc(stack, H, W, spec, row0, col0, cull_window if quad_keep is not None else None,
                     grad_flags=1 if (grad_culled_unwritten and quad_keep is not None) else 0)
        asum = torch.empty((T, H, W, 2), dtype=torch.float32, device=stack.device) if with_reg else None
        # (with_reg: every entry point that forms the sums clears them itself -- no second fill)
        sums = (torch.empty if with_reg else torch.zeros)(4, dtype=torch.float64, device=stack.device)
        reg_state = None
        if with_reg:
            # coverage masks / pair flags / sign words of the layer differences: written by the forward, read by the backward (include/vl3d.h)
            with torch.cuda.device(stack.device):
                reg_state = torch.empty(int(L.lib().vl3d_render_reg_state_bytes(desc)), dtype=torch.uint8, device=stack.device)
        # variant bits 12-15: 1 = keep the two-pass forward with regularisers (render, then the sums kernel) for A/B and cross-checks
        fused_reg = with_reg and ((int(spec.variant) >> 12) & 0xf) != 1
        qmap = _qmap(quad_keep, spec)
        with torch.cuda.device(stack.device):
            if fused_reg:
                # render + smoothness sums in ONE sweep over the stack (tile-culled model: the slot-by-slot regulariser kernel composites the
                # render from the samples it takes)
                L.check(L.lib().vl3d_render_fwd_reg(desc, L.ptr(stack), L.ptr(homos), *qmap, L.ptr(rgb), L.ptr(alpha), L.ptr(asum), L.ptr(sums),
                                                    L.ptr(reg_state), L.stream_ptr(stack.device)), "vl3d_render_fwd_reg")
            else:
                cull = None if quad_keep is None else _cull_scratch(desc, stack.device)
                L.check(L.lib().vl3d_render_fwd(desc, L.ptr(stack), L.ptr(homos), *qmap, L.ptr(cull), L.ptr(rgb), L.ptr(alpha), L.ptr(asum),
                                                L.stream_ptr(stack.device)), "vl3d_render_fwd")
        ctx.save_for_backward(stack, homos, rgb, alpha)
        ctx.quad_keep = quad_keep
        ctx.spec = spec
        ctx.reg_state = reg_state
        ctx.desc = desc
        ctx.with_reg = with_reg
        if with_reg and not fused_reg:
            with torch.cuda.device(stack.device):
                L.check(L.lib().vl3d_render_reg_fwd(desc, L.ptr(stack), L.ptr(homos), *qmap, L.ptr(sums), L.ptr(reg_state),
                                                    L.stream_ptr(stack.device)), "vl3d_render_reg_fwd")
        if asum is None:
            asum = torch.zeros((0,), dtype=torch.float32, device=stack.device)
        return rgb, alpha, sums.to(torch.float32), asum

    @staticmethod
    def backward(ctx, g_rgb, g_alpha, g_sums, g_asum):
        if ctx.nothing_to_render:
            return (torch.zeros_like(ctx.saved_tensors[0]), torch.zeros((ctx.saved_tensors[0].shape[0], 3, 3), dtype=ctx.homos_like[0],
                                                                        device=ctx.homos_like[1]) if ctx.cam else None) + (None,) * 10
        stack, homos, rgb, alpha = ctx.saved_tensors
        g_reg = g_sums.to(torch.float32).contiguous() if (ctx.with_reg and g_sums is not None) else None
        g_asum = g_asum.to(torch.float32).contiguous() if (ctx.with_reg and g_asum is not None) else None
        g_rgb = g_rgb.contiguous() if g_rgb is not None else torch.zeros_like(rgb)
        g_alpha = g_alpha.contiguous() if g_alpha is not None else None
        g_homos = None
        if ctx.cam:
            # beside the stack backward, from the same saved outputs and output gradients; [D,3,3] in the dtype and on the device of the `homos` passed in
            gh = torch.empty((stack.shape[0], 3, 3), dtype=torch.float32, device=stack.device)
            with torch.cuda.device(stack.device):
                nb = int(L.lib().vl3d_render_bwd_homos_scratch_bytes(ctx.desc))
                cam_scratch = torch.empty((nb + 3) // 4, dtype=torch.float32, device=stack.device)
                L.check(L.lib().vl3d_render_bwd_homos(ctx.desc, L.ptr(stack), L.ptr(homos), *_qmap(ctx.quad_keep, ctx.spec), L.ptr(rgb), L.ptr(alpha),
                                                      L.ptr(g_rgb), L.ptr(g_alpha), L.ptr(gh), L.ptr(cam_scratch), nb, L.stream_ptr(stack.device)),
                        "vl3d_render_bwd_homos")
            g_homos = gh.to(device=ctx.homos_like[1], dtype=ctx.homos_like[0])
            if not ctx.needs_input_grad[0]:      # a frozen stack (pose refinement): no stack backward at all
                return (None, g_homos) + (None,) * 10
        global LAST_BWD_SCRATCH, LAST_BWD_CALL
        LAST_BWD_CALL = (ctx.desc, "render" if ctx.fused_adam is None else "adam",
                         (ctx.quad_keep if ctx.fused_adam is None else ctx.fused_adam.quad_keep) is not None, g_reg is not None or g_asum is not None,
                         None)      # (the fused step's scratch is the optimiser's: at least vl3d_render_bwd_scratch_bytes, or the entry refuses)
        if ctx.fused_adam is not None:
            # backward + optimiser step in one pass over the window (vl3d_render_bwd_adam): no gradient tensor exists afterwards
            LAST_BWD_SCRATCH = ctx.fused_adam.backward_step(ctx.desc, ctx.leaf, homos, rgb, alpha, g_rgb, g_alpha, g_reg, ctx.reg_state, g_asum)
            return (None,) * 12
        g_stack = torch.empty(stack.shape, dtype=stack.dtype, device=stack.device)     # the gradient has the stack's dtype in the ABI
        with torch.cuda.device(stack.device):
            nscratch = int(L.lib().vl3d_render_bwd_scratch_bytes(ctx.desc))
            # every word the kernels read is written by the plan kernels of the same call, the header included (bwd_plan_k): nothing to clear
            scratch = torch.empty((nscratch + 3) // 4, dtype=torch.float32, device=stack.device)
            LAST_BWD_CALL = LAST_BWD_CALL[:4] + (nscratch,)
            if (ctx.desc.variant & 0xf) == 1 or ctx.desc.uv_noise_seed:      # (no plan kernel will write the header: the diagnostic word reads 0)
                scratch[:16].zero_()
            L.check(L.lib().vl3d_render_bwd(ctx.desc, L.ptr(stack), L.ptr(homos), *_qmap(ctx.quad_keep, ctx.spec), L.ptr(rgb), L.ptr(alpha),
                                            L.ptr(g_rgb), L.ptr(g_alpha), L.ptr(g_reg), L.ptr(ctx.reg_state), L.ptr(g_asum), L.ptr(g_stack),
                                            L.ptr(scratch), nscratch, L.stream_ptr(stack.device)), "vl3d_render_bwd")
        LAST_BWD_SCRATCH = scratch
        return (g_stack, g_homos) + (None,) * 10


def _check_camera_grad(stack, spec, with_reg, fused_adam, quad_keep, cull_window):
    """what render_planes refuses when `homos` requires a gradient: what vl3d_render_bwd_homos is not built for (include/vl3d.h), and the two
    callers whose camera gradient would be wrong rather than missing."""
    who = "render_planes: homos.requires_grad (the camera gradient)"
    if with_reg:
        raise RuntimeError(f"{who} is not built for the regulariser sums: they depend on the coordinates too, and their camera gradient does not exist")
    if fused_adam is not None:
        raise RuntimeError(f"{who} cannot ride the fused optimiser step: vl3d_render_bwd_adam rewrites the texels the camera gradient reads")
    if spec.coord_mode == "affine_planes":
        raise RuntimeError(f"{who} is not built for per-plane records (coord_mode 'affine_planes')")
    if stack.dtype != torch.float32:
        raise RuntimeError(f"{who} is built for float32 stacks only, got {stack.dtype}")
    if getattr(spec, "tile", (0, 0))[0]:
        raise RuntimeError(f"{who} is not built for the tile-exact layout (RenderSpec.tile)")
    if getattr(spec, "uv_noise_seed", 0):
        raise RuntimeError(f"{who} is not built for add_uv_noise (uv_noise_seed = 0)")
    if cull_window is not None and quad_keep is not None:
        raise RuntimeError(f"{who} takes the whole plane: no cull_window")
    if int(spec.variant) != 0:
        raise RuntimeError(f"{who} has no kernel variants (spec.variant = 0)")
    conv = (spec.coord_mode, spec.border, spec.act_order)
    if conv not in (("affine", "hardcut", "post"), ("utils_mpi", "zeros", "pre")):
        raise RuntimeError(f"{who} is built for the planar convention (affine, hardcut, post) and the utils_mpi one (utils_mpi, zeros, pre), got {conv}")


def mask_channel_supported(stack, spec):
    """the descriptors vl3d_render_fwd_mask / _bwd_mask are built for (include/vl3d.h): the planar convention stage 1 ships."""
    return (spec.coord_mode == "affine" and spec.border == "hardcut" and spec.act_order == "post" and spec.rgb_act == "sigmoid"
            and spec.alpha_act == "sigmoid" and stack.dtype == torch.float32)


class _RenderPlanesMask(torch.autograd.Function):
    """render (+ layer regularisers) with stage 1's loop mask as a fifth composited channel (MPI.py:568-583): one forward and one backward
    sweep over the stack for colours, regularisers and label; the label's gradient reaches the mask texture only (detached weights).
    `homos` gets no gradient here: render_planes is the camera-differentiable entry."""

    @staticmethod
    def forward(ctx, stack, mask, homos, H, W, spec, with_reg):
        ctx.set_materialize_grads(False)      # outputs the loss does not use come back as None, not as zero-filled tensors (a fill each, and reads in the backward kernels)
        L.check_cuda(stack, mask, homos)
        D, T, Hs, Ws, _ = stack.shape
        if tuple(mask.shape) not in ((D, T, Hs, Ws), (D, T, Hs, Ws, 1)) or mask.dtype != torch.float32:
            raise RuntimeError(f"the loop-mask texture must be float32 [D,T,Hs,Ws] = {(D, T, Hs, Ws)}, got {tuple(mask.shape)} {mask.dtype}")
        if homos.shape != (D, 3, 3):
            raise RuntimeError(f"homos must be [D,3,3] = [{D},3,3], got {tuple(homos.shape)}")
        stack, mask = stack.contiguous(), mask.contiguous()
        homos = homos.detach().to(torch.float32).contiguous()
        dev = stack.device
        rgb = torch.empty((T, H, W, 3), dtype=torch.float32, device=dev)
        alpha = torch.empty((T, H, W), dtype=torch.float32, device=dev)
        label = torch.empty((T, H, W), dtype=torch.float32, device=dev)
        desc = _desc(stack, H, W, spec, 0, 0)
        asum = torch.empty((T, H, W, 2), dtype=torch.float32, device=dev) if with_reg else None
        sums = torch.empty(4, dtype=torch.float64, device=dev) if with_reg else None      # (cleared by vl3d_render_fwd_mask)
        reg_state = None
        with torch.cuda.device(dev):
            if with_reg:
                reg_state = torch.empty(int(L.lib().vl3d_render_reg_state_bytes(desc)), dtype=torch.uint8, device=dev)
            L.check(L.lib().vl3d_render_fwd_mask(desc, L.ptr(stack), L.ptr(mask), L.ptr(homos), L.ptr(rgb), L.ptr(alpha), L.ptr(label), L.ptr(asum),
                                                 L.ptr(sums), L.ptr(reg_state), L.stream_ptr(dev)), "vl3d_render_fwd_mask")
        ctx.save_for_backward(stack, mask, homos, rgb, alpha)
        ctx.desc, ctx.reg_state, ctx.with_reg = desc, reg_state, with_reg
        z = torch.zeros((0,), dtype=torch.float32, device=dev)
        return rgb, alpha, label, (sums.to(torch.float32) if with_reg else z), (asum if with_reg else z)

    @staticmethod
    def backward(ctx, g_rgb, g_alpha, g_label, g_sums, g_asum):
        stack, mask, homos, rgb, alpha = ctx.saved_tensors
        dev = stack.device
        g_reg = g_sums.to(torch.float32).contiguous() if (ctx.with_reg and g_sums is not None) else None
        g_asum = g_asum.to(torch.float32).contiguous() if (ctx.with_reg and g_asum is not None) else None
        g_rgb = g_rgb.contiguous() if g_rgb is not None else torch.zeros_like(rgb)
        g_alpha = g_alpha.contiguous() if g_alpha is not None else None
        g_label = g_label.contiguous() if g_label is not None else torch.zeros_like(alpha)
        g_stack = torch.empty_like(stack)
        g_mask = torch.empty_like(mask)
        with torch.cuda.device(dev):
            nscratch = int(L.lib().vl3d_render_bwd_scratch_bytes(ctx.desc))
            scratch = torch.empty((nscratch + 3) // 4, dtype=torch.float32, device=dev)
            if (ctx.desc.variant & 0xf) == 1:
                scratch[:16].zero_()
            L.check(L.lib().vl3d_render_bwd_mask(ctx.desc, L.ptr(stack), L.ptr(mask), L.ptr(homos), L.ptr(rgb), L.ptr(alpha), L.ptr(g_rgb), L.ptr(g_alpha),
                                                 L.ptr(g_label), L.ptr(g_reg), L.ptr(ctx.reg_state), L.ptr(g_asum), L.ptr(g_stack), L.ptr(g_mask),
                                                 L.ptr(scratch), nscratch, L.stream_ptr(dev)), "vl3d_render_bwd_mask")
        global LAST_BWD_SCRATCH, LAST_BWD_CALL
        LAST_BWD_SCRATCH = scratch
        LAST_BWD_CALL = (ctx.desc, "mask", False, g_reg is not None or g_asum is not None, nscratch)
        return g_stack, g_mask, None, None, None, None, None


def render_planes_with_mask(stack, mask, homos, H, W, spec: RenderSpec = RenderSpec(), with_regularisers=False):
    """-> (rgb [T,H,W,3], alpha [T,H,W], label [T,H,W], smooth_sums[4], alpha_sums [T,H,W,2]) -- render_planes (with_regularisers: plus
    render_planes_with_regularisers' sums) and the composited loop-mask label `sum_k w_k sigmoid(sample(mask_k))` of MPI.py:568-583 from the
    same pass; `mask` [D,T,Hs,Ws] logits.  Needs mask_channel_supported(stack, spec)."""
    if spec.act_order == "baked":
        raise RuntimeError("the loop-mask channel is not built for the bake rule (act_order='baked'): stage 1 trains under 'post'")
    return _RenderPlanesMask.apply(stack, mask, homos, int(H), int(W), spec, bool(with_regularisers))


class _LabelNoise(torch.autograd.Function):
    """MPI.py:568-583 under add_uv_noise (MPI.py:519-522): the loop-mask texture sampled at the UNJITTERED positions, composited with the detached
    alphas of the JITTERED colour samples (vl3d_label_noise_fwd / _bwd: the jitter field of spec.uv_noise_seed, the colour pass's).  Gradient to the mask only."""

    @staticmethod
    def forward(ctx, mask, stack, homos, H, W, spec):
        L.check_cuda(mask, stack, homos)
        D, T, Hs, Ws, _ = stack.shape
        if tuple(mask.shape) != (D, T, Hs, Ws) or mask.dtype != torch.float32 or stack.dtype != torch.float32:
            raise RuntimeError(f"loop-mask label: float32 stack (D,T,Hs,Ws,4) and mask [D,T,Hs,Ws] = {(D, T, Hs, Ws)}, got {tuple(mask.shape)} {mask.dtype}")
        if homos.shape != (D, 3, 3):
            raise RuntimeError(f"homos must be [D,3,3] = [{D},3,3], got {tuple(homos.shape)}")
        stack, mask = stack.detach().contiguous(), mask.detach().contiguous()
        homos = homos.detach().to(torch.float32).contiguous()
        desc = _desc(stack, H, W, spec, 0, 0)
        label = torch.empty((T, H, W), dtype=torch.float32, device=stack.device)
        with torch.cuda.device(stack.device):
            L.check(L.lib().vl3d_label_noise_fwd(desc, L.ptr(stack), L.ptr(mask), L.ptr(homos), L.ptr(label), L.stream_ptr(stack.device)), "vl3d_label_noise_fwd")
        ctx.save_for_backward(stack, mask, homos)
        ctx.desc = desc
        return label

    @staticmethod
    def backward(ctx, g):
        stack, mask, homos = ctx.saved_tensors
        g = g.contiguous()
        gm = torch.empty_like(mask)
        with torch.cuda.device(stack.device):
            L.check(L.lib().vl3d_label_noise_bwd(ctx.desc, L.ptr(stack), L.ptr(mask), L.ptr(homos), L.ptr(g), L.ptr(gm), L.stream_ptr(stack.device)), "vl3d_label_noise_bwd")
        return gm, None, None, None, None, None


def loop_mask_label_with_uv_noise(mask, stack, homos, H, W, spec: RenderSpec):
    """label [T,H,W] = sum_k w_k sigmoid(sample(mask_k)) with the mask sampled at the plain positions and the weights w_k = a_k T_k from the alphas at
    the positions jittered by spec.uv_noise_seed's field (MPI.py:519-522, 568-583).  mask [D,T,Hs,Ws] logits (receives the gradient), stack detached."""
    return _LabelNoise.apply(mask, stack, homos, int(H), int(W), spec)


def render_frame_run(stack, frame0, nframes, homos, H, W, spec: RenderSpec = RenderSpec(), out=None, quad_keep=None):
    """Evaluation render (no gradient) of frames frame0 .. frame0 + nframes - 1 of the clip `stack` [D,T,Hs,Ws,4], read IN PLACE
    (vl3d_render_fwd_frames) -> (rgb [n,H,W,3], alpha [n,H,W]): `render_planes(stack[:, ts], ...)` gathers the frames first -- 571 MB per
    720p frame at D = 32 on 1.1x planes, more than the render reads.  `out`: an (rgb, alpha) pair of buffers to write into; `quad_keep`
    [D,QH,QW]: a tile-culled model (a sample inside a culled quad is not covered, as in render_planes(quad_keep=...))."""
    L.check_cuda(stack, homos)
    D, T = stack.shape[:2]
    if not stack.is_contiguous() or stack.dtype not in (torch.float32, torch.float16):
        raise RuntimeError("render_frame_run: a contiguous float32 / float16 clip [D,T,Hs,Ws,4]")
    if not (0 <= frame0 and nframes >= 1 and frame0 + nframes <= T):
        raise RuntimeError(f"render_frame_run: frames {frame0} .. {frame0 + nframes - 1} leave the clip of {T}")
    if homos.shape != (D, 3, 3):
        raise RuntimeError(f"homos must be [D,3,3] = [{D},3,3], got {tuple(homos.shape)}")
    homos = homos.detach().to(torch.float32).contiguous()
    desc = _desc(stack, H, W, spec, 0, 0)
    desc.T = int(nframes)
    rgb, alpha = _out_buffers(out, nframes, H, W, stack.device, "render_frame_run")
    with torch.cuda.device(stack.device):
        qk = None if quad_keep is None else _quad_map(quad_keep, D)
        cull = None if qk is None else _cull_scratch(desc, stack.device)
        L.check(L.lib().vl3d_render_fwd_frames(desc, L.ptr(stack), int(frame0), int(T), L.ptr(homos), *_qmap(qk, spec), L.ptr(cull), L.ptr(rgb),
                                               L.ptr(alpha), L.stream_ptr(stack.device)), "vl3d_render_fwd_frames")
    return rgb, alpha


def _path_indices(frame_cam, frame_t, n_cams, T, device, who):
    """the (camera, frame) indices of a camera path, range-checked on the host (the kernels cannot report a bad index: they skip its frame)
    and uploaded in ONE pinned copy -> (N, int32 [2,N] on `device`: row 0 the cameras, row 1 the frames)."""
    import numpy as np
    cam, t = np.asarray(frame_cam).reshape(-1), np.asarray(frame_t).reshape(-1)
    if len(cam) != len(t):
        raise RuntimeError(f"{who}: frame_cam and frame_t name the same output frames ({len(cam)} cameras, {len(t)} frames)")
    if len(cam) == 0:
        raise RuntimeError(f"{who}: an empty path (N = 0 output frames)")
    if cam.dtype.kind not in "iu" or t.dtype.kind not in "iu":
        raise RuntimeError(f"{who}: frame_cam and frame_t are integer indices")
    if int(cam.min()) < 0 or int(cam.max()) >= n_cams:
        raise IndexError(f"{who}: camera index {int(cam.min())} .. {int(cam.max())} outside the {n_cams} cameras of homos")
    if int(t.min()) < 0 or int(t.max()) >= T:
        raise IndexError(f"{who}: frame index {int(t.min())} .. {int(t.max())} outside the clip of {T} frames")
    idx = torch.from_numpy(np.stack([cam, t]).astype(np.int32)).pin_memory().to(device, non_blocking=True)
    return len(cam), idx


def _time_indices(frame_cam, frame_time, n_cams, T, device, who):
    """the (camera, loop time) pairs of a path in loop time, checked on the host (the kernels cannot report a bad value: they skip its frame)
    and uploaded in ONE pinned copy -> (N, int32 [2,N] on `device`: row 0 the cameras, row 1 the BITS of the float32 times).  The times are
    cast to float32 first and must then be finite and in [0, T) (baked.loop_times reduces any real time): ValueError."""
    import numpy as np
    cam, t = np.asarray(frame_cam).reshape(-1), np.asarray(frame_time).reshape(-1)
    if len(cam) != len(t):
        raise RuntimeError(f"{who}: frame_cam and frame_time name the same output frames ({len(cam)} cameras, {len(t)} times)")
    if len(cam) == 0:
        raise RuntimeError(f"{who}: an empty path (N = 0 output frames)")
    if cam.dtype.kind not in "iu" or t.dtype.kind not in "iuf":
        raise RuntimeError(f"{who}: frame_cam are integer indices, frame_time real loop times")
    if int(cam.min()) < 0 or int(cam.max()) >= n_cams:
        raise IndexError(f"{who}: camera index {int(cam.min())} .. {int(cam.max())} outside the {n_cams} cameras of homos")
    t = t.astype(np.float32)
    if not np.isfinite(t).all():
        raise ValueError(f"{who}: a loop time is not finite")
    if float(t.min()) < 0 or float(t.max()) >= T:
        raise ValueError(f"{who}: loop time {float(t.min())} .. {float(t.max())} outside [0, {T}) (baked.loop_times reduces any time into the loop)")
    idx = torch.from_numpy(np.stack([cam.astype(np.int32), t.view(np.int32)])).pin_memory().to(device, non_blocking=True)
    return len(cam), idx


def _path_cull_scratch(desc, n_cams, device, cull_scratch, who):
    """the plane masks of a path render, [n_cams][tiles][2] uint64 (vl3d_render_path_cull_scratch_bytes): the caller's buffer checked for
    device, dtype and size, or a fresh one; call under torch.cuda.device(device)."""
    need = int(L.lib().vl3d_render_path_cull_scratch_bytes(desc, int(n_cams)))
    if cull_scratch is None:
        return torch.empty((need + 7) // 8, dtype=torch.int64, device=device)
    if not isinstance(cull_scratch, torch.Tensor) or not cull_scratch.is_cuda or cull_scratch.device != device:
        raise RuntimeError(f"{who}: cull_scratch must be a tensor on the model's device")
    if cull_scratch.dtype != torch.int64 or not cull_scratch.is_contiguous() or cull_scratch.numel() * 8 < need:
        raise RuntimeError(f"{who}: cull_scratch must be contiguous int64 of at least {need} bytes "
                           f"(vl3d_render_path_cull_scratch_bytes: two 64-bit plane masks per camera and 64 x 8 pixel tile)")
    return cull_scratch


def _baked_dense(who, baked, homos, spec, quad_keep):
    """the dense source of a baked render, validated: the clip [D,T,Hs,Ws,4] uint8 with its optional quad map -> (T, the source half of the call)"""
    L.check_cuda(baked, homos)
    if baked.requires_grad or (torch.is_grad_enabled() and homos.requires_grad):
        raise RuntimeError(f"{who}: baked texels have no backward (train the float model, then bake it)")
    if baked.dtype != torch.uint8 or baked.dim() != 5 or baked.shape[4] != 4 or not baked.is_contiguous():
        raise RuntimeError(f"{who}: a contiguous uint8 clip [D,T,Hs,Ws,4] (baked.bake_texels)")
    if spec.coord_mode != "affine" or spec.border != "hardcut":
        raise RuntimeError("a baked model renders in the planar MPV convention (RenderSpec.mpv())")
    if getattr(spec, "tile", (0, 0))[0] and quad_keep is None:
        raise RuntimeError("RenderSpec.tile (tile-exact layout) belongs to a tile-culled model: pass its quad_keep map")
    D, T, Hs, Ws = baked.shape[:4]
    qk = None if quad_keep is None else _quad_map(quad_keep, D)
    return T, types.SimpleNamespace(entry="vl3d_render_fwd_baked", dims=(D, Hs, Ws), device=baked.device, qk=qk, head=(L.ptr(baked), int(T)), culled=())


def _baked_pool(who, layout, pool, homos, spec, quad_keep, culled_rgba8):
    """the pool source of a baked render, validated: the kernel trusts the block table, so the table and the quad map are checked here against
    the layout's own dimensions -> (T, the source half of the call)"""
    L.check_cuda(pool, homos, layout.blocks)
    if pool.requires_grad or (torch.is_grad_enabled() and homos.requires_grad):
        raise RuntimeError(f"{who}: baked texels have no backward (train the float model, then bake it)")
    if pool.dtype != torch.uint8 or pool.dim() != 2 or pool.shape[1] != 4 or not pool.is_contiguous() or pool.shape[0] != layout.n_slots * 64:
        raise RuntimeError(f"{who}: a contiguous uint8 pool [n_slots * 64, 4] of the layout (baked.bake_pool)")
    if spec.coord_mode != "affine" or spec.border != "hardcut":
        raise RuntimeError("a baked model renders in the planar MPV convention (RenderSpec.mpv())")
    if quad_keep is None:
        raise RuntimeError(f"{who}: the quad map the block table was built from (quad_keep [D,QH,QW]) is required")
    D = layout.D
    qk = _quad_map(quad_keep, D)
    grid = getattr(layout, "quad_grid", None)      # (a layout object made before PackedLayout recorded its grid: nothing to compare with)
    if grid is not None and tuple(quad_keep.shape[1:]) != tuple(grid):
        raise RuntimeError(f"quad_keep is {tuple(quad_keep.shape[1:])} quads per plane, the layout's block table was built from {tuple(grid)}")
    bl = layout.blocks
    if bl.dtype != torch.int32 or not bl.is_contiguous() or tuple(bl.shape) != (D, -(-layout.Hs // 8), -(-layout.Ws // 8)) or bl.device != pool.device:
        raise RuntimeError(f"{who}: the layout's block table must be contiguous int32 [D, ceil(Hs/8), ceil(Ws/8)] on the pool's device")
    if bool(getattr(spec, "tile", (0, 0))[0]) != (layout.tile is not None):
        raise RuntimeError(f"{who}: RenderSpec.tile and the layout's tile must both name the tile-exact layout, or neither")
    return layout.T, types.SimpleNamespace(entry="vl3d_render_fwd_baked_pool", dims=(D, layout.Hs, layout.Ws), device=pool.device, qk=qk,
                                           head=(L.ptr(bl), L.ptr(pool), int(layout.T)), culled=(int(culled_rgba8) & 0xFFFFFFFF,))


def _baked_render(who, src, n, frame0, path, homos, H, W, spec, out, frames8, bg, cull_scratch=None, by_time=False):
    """the one call of the six baked renders: `n` output frames of source `src` (_baked_dense / _baked_pool) -- the run from `frame0` under
    homos [D,3,3], or the `path` (C, idx [2,n] on the device) under homos [C,D,3,3] -- into the float sink (`out`, or fresh buffers) or the
    display sink (`frames8`, `bg`).  Fills vl3d_baked_frames and vl3d_baked_out and calls src.entry; `by_time`: the path's second row holds
    float32 loop times (_time_indices): vl3d_baked_times and the entry's `_times` form."""
    dev = src.device
    homos = homos.detach().to(torch.float32).contiguous()
    desc = _desc_dims(src.dims[0], n, src.dims[1], src.dims[2], H, W, spec, L.STACK_DTYPE["u8"])
    sel, sink, entry = L.BakedFrames(frame0=int(frame0)), L.BakedOut(), src.entry
    if by_time:
        sel, entry = L.BakedTimes(n_cams=path[0], frame_cam=path[1][0].data_ptr(), frame_time=path[1][1].data_ptr()), src.entry + "_times"
    elif path is not None:
        sel.n_cams, sel.frame_cam, sel.frame_t = path[0], path[1][0].data_ptr(), path[1][1].data_ptr()
    if frames8 is not None:
        sink.channels, bgc = _display_out(out, frames8, bg, n, H, W, dev, who)
        sink.frames, sink.bg, ret = frames8.data_ptr(), (None if bgc is None else L.C.addressof(bgc)), frames8
    else:
        ret = _out_buffers(out, n, H, W, dev, who)
        sink.rgb, sink.alpha = ret[0].data_ptr(), ret[1].data_ptr()
    with torch.cuda.device(dev):
        cull = None
        if src.qk is not None:
            cull = _cull_scratch(desc, dev) if path is None else _path_cull_scratch(desc, path[0], dev, cull_scratch, who)
        grid = (0, 0) if src.qk is None else _qgrid(src.qk, spec)
        L.check(getattr(L.lib(), entry)(desc, *src.head, L.ptr(homos), sel, L.ptr(src.qk), *grid, *src.culled, L.ptr(cull), sink,
                                        L.stream_ptr(dev)), entry)
    return ret


def _check_run(who, frame0, nframes, T, homos, D, of):
    """a run of one camera: frames inside the T of the source (`of`: how the message names it), homos [D,3,3]"""
    if not (0 <= frame0 and nframes >= 1 and frame0 + nframes <= T):
        raise RuntimeError(f"{who}: frames {frame0} .. {frame0 + nframes - 1} leave the {of} {T}")
    if homos.shape != (D, 3, 3):
        raise RuntimeError(f"homos must be [D,3,3] = [{D},3,3], got {tuple(homos.shape)}")


def _check_path(who, frame_cam, frame_t, T, homos, D, device):
    """a camera path: homos [C,D,3,3], the indices range-checked and uploaded -> (n output frames, (C, idx [2,n] int32 on `device`))"""
    if homos.dim() != 4 or tuple(homos.shape[1:]) != (D, 3, 3) or homos.shape[0] < 1:
        raise RuntimeError(f"homos must be [C,D,3,3] = [C,{D},3,3] with C >= 1 cameras, got {tuple(homos.shape)}")
    C = int(homos.shape[0])
    n, idx = _path_indices(frame_cam, frame_t, C, T, device, who)
    return n, (C, idx)


def _check_times(who, frame_cam, frame_time, T, homos, D, device):
    """a camera path in loop time: homos [C,D,3,3], cameras and times checked and uploaded -> (n output frames, (C, idx [2,n] on `device`))"""
    if homos.dim() != 4 or tuple(homos.shape[1:]) != (D, 3, 3) or homos.shape[0] < 1:
        raise RuntimeError(f"homos must be [C,D,3,3] = [C,{D},3,3] with C >= 1 cameras, got {tuple(homos.shape)}")
    C = int(homos.shape[0])
    n, idx = _time_indices(frame_cam, frame_time, C, T, device, who)
    return n, (C, idx)


def _check_bg(who, frames8, bg):
    if bg is not None and frames8 is None:
        raise ValueError(f"{who}: `bg` belongs to the display frames (`frames8=`)")


def render_frame_run_baked(baked, frame0, nframes, homos, H, W, spec: RenderSpec, out=None, quad_keep=None, frames8=None, bg=None):
    """render_frame_run on the BAKED texels of a playback model (videoloop3d_amd/baked.py; vl3d_render_fwd_baked): `baked` [D,T,Hs,Ws,4] uint8 --
    activated, times 255, truncated (baked.bake_texels) -- filtered bilinearly AFTER the activation, as a player filters the exported 8-bit
    atlases; nothing is activated behind the blend, so spec.rgb_act / alpha_act / act_order are not read.  Coverage (hard cut, culled quads,
    tile-exact layout) is decided by the float kernels' own code.  The planar convention only (RenderSpec.mpv()); forward only -- a baked
    model is not trained: inputs that require a gradient are refused (`homos` included: render_planes is the camera-differentiable entry).
    -> (rgb [n,H,W,3], alpha [n,H,W]) float32.
    `frames8` (uint8 [n,H,W,3|4] on the device): the DISPLAY frames instead -- baked.display_frames(rgb, alpha, bg, channels), byte for byte,
    written by the render launch (the display sink of vl3d_baked_out); no float output exists and `frames8` is returned.  `bg`: the background
    colour, 3 floats, or None."""
    who = "render_frame_run_baked"
    _check_bg(who, frames8, bg)
    T, src = _baked_dense(who, baked, homos, spec, quad_keep)
    _check_run(who, frame0, nframes, T, homos, src.dims[0], "clip of")
    return _baked_render(who, src, int(nframes), frame0, None, homos, H, W, spec, out, frames8, bg)


def render_frame_run_baked_pool(layout, pool, frame0, nframes, homos, H, W, spec: RenderSpec, out=None, *, quad_keep, culled_rgba8, frames8=None,
                                bg=None):
    """render_frame_run_baked from the baked POOL of a packed tile-culled model (baked.BakedPool; vl3d_render_fwd_baked_pool): `layout` the
    packed.PackedLayout whose block table addresses `pool` [n_slots * 64, 4] uint8 (8 x 8-texel blocks of baked RGBA8 texels), `quad_keep`
    [D,QH,QW] the quad map the table was built from, `culled_rgba8` the texel (r | g << 8 | b << 16 | a << 24) a block without storage reads
    as (BakedPool.culled_rgba8) -- both required, by keyword.  The kernel trusts the table: the layout's table and the quad map are checked
    here against the layout's own dimensions.  Frames frame0 .. frame0 + nframes - 1 of the model's layout.T -> (rgb [n,H,W,3], alpha [n,H,W]) float32: the bits of
    render_frame_run_baked on the unpacked texels, without the dense clip.  The planar convention only; forward only.  `frames8`, `bg`: the
    display frames instead, as render_frame_run_baked takes them."""
    who = "render_frame_run_baked_pool"
    _check_bg(who, frames8, bg)
    T, src = _baked_pool(who, layout, pool, homos, spec, quad_keep, culled_rgba8)
    _check_run(who, frame0, nframes, T, homos, src.dims[0], "model's")
    return _baked_render(who, src, int(nframes), frame0, None, homos, H, W, spec, out, frames8, bg)


def render_path_baked(baked, frame_cam, frame_t, homos, H, W, spec: RenderSpec, out=None, quad_keep=None, cull_scratch=None, frames8=None, bg=None):
    """A camera path on the baked clip (vl3d_render_fwd_baked with a path selection): N output frames in ONE plan launch plus ONE render launch,
    output frame i being frame frame_t[i] of `baked` [D,T,Hs,Ws,4] uint8 seen by camera frame_cam[i] of `homos` [C,D,3,3] -- the spiral of the offline
    renderer, where render_frame_run_baked takes one camera per call.  frame_cam / frame_t: host sequences or numpy arrays of N indices (checked
    here: IndexError).  `cull_scratch`: an int64 buffer of vl3d_render_path_cull_scratch_bytes to hold the plane masks [C][tiles][2] across calls (a
    tile-culled model; allocated per call when absent).  -> (rgb [N,H,W,3], alpha [N,H,W]) float32, frame i bit-equal to
    render_frame_run_baked(baked, frame_t[i], 1, homos[frame_cam[i]], ...).  Everything else as render_frame_run_baked, `frames8` / `bg` (the
    display frames uint8 [N,H,W,3|4] instead) included."""
    who = "render_path_baked"
    _check_bg(who, frames8, bg)
    T, src = _baked_dense(who, baked, homos, spec, quad_keep)
    n, path = _check_path(who, frame_cam, frame_t, T, homos, src.dims[0], src.device)
    return _baked_render(who, src, n, 0, path, homos, H, W, spec, out, frames8, bg, cull_scratch)


def render_path_baked_pool(layout, pool, frame_cam, frame_t, homos, H, W, spec: RenderSpec, out=None, *, quad_keep, culled_rgba8, cull_scratch=None,
                           frames8=None, bg=None):
    """render_path_baked from the baked POOL (vl3d_render_fwd_baked_pool with a path selection): `layout`, `pool`, `quad_keep`, `culled_rgba8` as
    render_frame_run_baked_pool takes them, the path as render_path_baked takes it.  -> (rgb [N,H,W,3], alpha [N,H,W]) float32, frame i bit-equal
    to render_frame_run_baked_pool(layout, pool, frame_t[i], 1, homos[frame_cam[i]], ...).  `frames8`, `bg`: the display frames instead."""
    who = "render_path_baked_pool"
    _check_bg(who, frames8, bg)
    T, src = _baked_pool(who, layout, pool, homos, spec, quad_keep, culled_rgba8)
    n, path = _check_path(who, frame_cam, frame_t, T, homos, src.dims[0], src.device)
    return _baked_render(who, src, n, 0, path, homos, H, W, spec, out, frames8, bg, cull_scratch)


def render_times_baked(baked, frame_cam, frame_time, homos, H, W, spec: RenderSpec, out=None, quad_keep=None, cull_scratch=None, frames8=None, bg=None):
    """A camera path in LOOP TIME on the baked clip (vl3d_render_fwd_baked_times): render_path_baked with a real-valued time per output frame.
    The clip is a loop of T frames; output frame i shows it at time frame_time[i] in [0, T) -- the linear interpolation of its TEXELS between
    frame t0 = floor(time) and frame t1 = t0 + 1, which wraps to frame 0 behind the last frame, by f = time - t0 -- seen by camera frame_cam[i]
    of `homos` [C,D,3,3], in ONE plan launch plus ONE render launch.  A frame at an integer time has the bits of render_path_baked's frame
    (cam, t0).  frame_time: a host sequence or numpy array, finite and already in [0, T) as float32 (ValueError; baked.loop_times reduces any
    time); frame_cam as render_path_baked checks it (IndexError); both go up in one pinned copy.  Everything else -- `out`, `quad_keep`,
    `cull_scratch`, `frames8` / `bg` -- as render_path_baked."""
    who = "render_times_baked"
    _check_bg(who, frames8, bg)
    T, src = _baked_dense(who, baked, homos, spec, quad_keep)
    n, path = _check_times(who, frame_cam, frame_time, T, homos, src.dims[0], src.device)
    return _baked_render(who, src, n, 0, path, homos, H, W, spec, out, frames8, bg, cull_scratch, by_time=True)


def render_times_baked_pool(layout, pool, frame_cam, frame_time, homos, H, W, spec: RenderSpec, out=None, *, quad_keep, culled_rgba8, cull_scratch=None,
                            frames8=None, bg=None):
    """render_times_baked from the baked POOL (vl3d_render_fwd_baked_pool_times): `layout`, `pool`, `quad_keep`, `culled_rgba8` as
    render_frame_run_baked_pool takes them, cameras and times as render_times_baked takes them (the loop is the model's layout.T frames).  A
    static block serves both frames of a time from one fetch, a dynamic block is read at slot + t0 and slot + t1.  -> the bits of
    render_times_baked on the unpacked texels."""
    who = "render_times_baked_pool"
    _check_bg(who, frames8, bg)
    T, src = _baked_pool(who, layout, pool, homos, spec, quad_keep, culled_rgba8)
    n, path = _check_times(who, frame_cam, frame_time, T, homos, src.dims[0], src.device)
    return _baked_render(who, src, n, 0, path, homos, H, W, spec, out, frames8, bg, cull_scratch, by_time=True)


# ---- disparity (include/vl3d.h "Disparity"; csrc/vl3d_render_disp.hip) -------------------------------------------------------------------
def depth_rows(extrin, intrin, planedepth, normalise=None):
    """The affine rows of the inverse view depth (MPV.py:385, MPI.py:493: 1 / zbuf of the planar mesh): for the ref -> target extrinsic
    E = [R | t] that render() receives, the intrinsics K of the call (a crop's are the shifted ones) and plane depths z_k (plane 0 nearest),
        rho_k(x, y) = row_k . (x + c, y + c, 1),   row_k = (K^-T r3) / (z_k + r3 . t),   r3 the third COLUMN of R, c the pixel centre,
    formed on the host in float64.  extrin [4,4] with intrin [3,3] -> float32 [D,3]; extrin [C,4,4] with intrin [C,3,3] (or one [3,3] for all
    cameras) -> [C,D,3].  `normalise` = (near, far): stage 1's normalisation (MPI.py:494), (rho - 1 / far) / (1 / near - 1 / far), folded into
    the rows -- it is affine in rho, so the kernels do not know about it."""
    E = torch.as_tensor(extrin).detach().to("cpu", torch.float64)
    K = torch.as_tensor(intrin).detach().to("cpu", torch.float64)
    z = torch.as_tensor(planedepth).detach().to("cpu", torch.float64).reshape(-1)
    single = E.dim() == 2
    if tuple(E.shape[-2:]) != (4, 4) or E.dim() not in (2, 3) or tuple(K.shape[-2:]) != (3, 3) or K.dim() not in (2, 3):
        raise RuntimeError(f"depth_rows: extrin [4,4] or [C,4,4] and intrin [3,3] or [C,3,3], got {tuple(E.shape)} and {tuple(K.shape)}")
    E = E.reshape(-1, 4, 4)
    K = K.reshape(-1, 3, 3)
    if K.shape[0] not in (1, E.shape[0]) or (single and K.shape[0] != 1):
        raise RuntimeError(f"depth_rows: {E.shape[0]} extrinsics and {K.shape[0]} intrinsics")
    r3, t = E[:, :3, 2], E[:, :3, 3]
    num = (torch.linalg.inv(K).transpose(-1, -2) @ r3[..., None])[..., 0].expand(E.shape[0], 3)      # K^-T r3, [C,3]
    rows = num[:, None, :] / (z[None, :] + (r3 * t).sum(-1)[:, None])[..., None]                      # [C,D,3]
    if normalise is not None:
        near, far = float(normalise[0]), float(normalise[1])
        rows = rows.clone()
        rows[..., 2] -= 1.0 / far
        rows = rows / (1.0 / near - 1.0 / far)
    rows = rows.to(torch.float32)
    return rows[0] if single else rows


def _disp_buffers(out, n, H, W, device, who):
    """(disp [n,H,W], alpha [n,H,W]) float32: fresh, or the caller's `out` pair checked."""
    if out is None:
        return torch.empty((n, H, W), dtype=torch.float32, device=device), torch.empty((n, H, W), dtype=torch.float32, device=device)
    disp, alpha = out
    for b in (disp, alpha):
        if not isinstance(b, torch.Tensor) or b.device != device or b.dtype != torch.float32 or tuple(b.shape) != (n, H, W) or not b.is_contiguous():
            raise RuntimeError(f"{who}: `out` must be contiguous float32 (disp [n,H,W], alpha [n,H,W]) = [{n},{H},{W}] on the model's device")
    return disp, alpha


def _disp_rows(who, rows, homos, device):
    """rows [D,3] beside homos [D,3,3], or [C,D,3] beside [C,D,3,3], as contiguous float32 on `device`"""
    if not isinstance(rows, torch.Tensor) or tuple(rows.shape) != tuple(homos.shape[:-2]) + (3,):
        raise RuntimeError(f"{who}: rows must be {list(homos.shape[:-2]) + [3]} beside homos {list(homos.shape)} (render.depth_rows), "
                           f"got {tuple(rows.shape) if isinstance(rows, torch.Tensor) else type(rows).__name__}")
    return rows.detach().to(device=device, dtype=torch.float32).contiguous()


def render_frame_run_disparity(stack, frame0, nframes, homos, rows, H, W, spec: RenderSpec, quad_keep=None, out=None):
    """The disparity map of frames frame0 .. frame0 + nframes - 1 of the float clip `stack` [D,T,Hs,Ws,4] (float32 / float16), read in place
    as render_frame_run reads it (vl3d_render_disp_fwd): per pixel sum_k w_k rho_k with the colour composite's own blend weights w_k and
    rho_k = rows[k] . (x + c, y + c, 1) (depth_rows) -> (disp [n,H,W], alpha [n,H,W]) float32.  The planar convention only (RenderSpec.mpv(),
    sample-then-activate), every alpha_act; `quad_keep` [D,QH,QW]: a tile-culled model.  Forward only."""
    who = "render_frame_run_disparity"
    L.check_cuda(stack, homos)
    if stack.dim() != 5 or stack.shape[4] != 4 or not stack.is_contiguous() or stack.dtype not in (torch.float32, torch.float16):
        raise RuntimeError(f"{who}: a contiguous float32 / float16 clip [D,T,Hs,Ws,4]")
    D, T = stack.shape[:2]
    _check_run(who, frame0, nframes, T, homos, D, "clip of")
    if getattr(spec, "tile", (0, 0))[0] and quad_keep is None:
        raise RuntimeError("RenderSpec.tile (tile-exact layout) belongs to a tile-culled model: pass its quad_keep map")
    homos = homos.detach().to(torch.float32).contiguous()
    rows = _disp_rows(who, rows, homos, stack.device)
    desc = _desc(stack, H, W, spec, 0, 0)
    desc.T = int(nframes)
    disp, alpha = _disp_buffers(out, int(nframes), H, W, stack.device, who)
    with torch.cuda.device(stack.device):
        qk = None if quad_keep is None else _quad_map(quad_keep, D)
        cull = None if qk is None else _cull_scratch(desc, stack.device)
        L.check(L.lib().vl3d_render_disp_fwd(desc, L.ptr(stack), int(frame0), int(T), L.ptr(homos), L.ptr(rows), *_qmap(qk, spec), L.ptr(cull),
                                             L.ptr(disp), L.ptr(alpha), L.stream_ptr(stack.device)), "vl3d_render_disp_fwd")
    return disp, alpha


def _baked_disparity(who, src, n, frame0, path, homos, rows, H, W, spec, out, cull_scratch=None):
    """the one call of the four baked disparity renders: _baked_render with `rows` beside the homographies and (disp, alpha) for a sink"""
    dev = src.device
    homos = homos.detach().to(torch.float32).contiguous()
    rows = _disp_rows(who, rows, homos, dev)
    desc = _desc_dims(src.dims[0], n, src.dims[1], src.dims[2], H, W, spec, L.STACK_DTYPE["u8"])
    sel, entry = L.BakedFrames(frame0=int(frame0)), src.entry.replace("vl3d_render_fwd_", "vl3d_render_disp_")
    if path is not None:
        sel.n_cams, sel.frame_cam, sel.frame_t = path[0], path[1][0].data_ptr(), path[1][1].data_ptr()
    disp, alpha = _disp_buffers(out, n, H, W, dev, who)
    with torch.cuda.device(dev):
        cull = None
        if src.qk is not None:
            cull = _cull_scratch(desc, dev) if path is None else _path_cull_scratch(desc, path[0], dev, cull_scratch, who)
        grid = (0, 0) if src.qk is None else _qgrid(src.qk, spec)
        L.check(getattr(L.lib(), entry)(desc, *src.head, L.ptr(homos), L.ptr(rows), sel, L.ptr(src.qk), *grid, *src.culled, L.ptr(cull),
                                        L.ptr(disp), L.ptr(alpha), L.stream_ptr(dev)), entry)
    return disp, alpha


def render_frame_run_disparity_baked(baked, frame0, nframes, homos, rows, H, W, spec: RenderSpec, quad_keep=None, out=None):
    """render_frame_run_disparity on the baked clip of a playback model (vl3d_render_disp_baked): `baked`, the frames, `homos`, `quad_keep` as
    render_frame_run_baked takes them, `rows` [D,3] (depth_rows).  Alpha is the bilinear blend of the decoded alpha bytes, nothing activated:
    the alpha returned has the bits of render_frame_run_baked's.  -> (disp [n,H,W], alpha [n,H,W]) float32."""
    who = "render_frame_run_disparity_baked"
    T, src = _baked_dense(who, baked, homos, spec, quad_keep)
    _check_run(who, frame0, nframes, T, homos, src.dims[0], "clip of")
    return _baked_disparity(who, src, int(nframes), frame0, None, homos, rows, H, W, spec, out)


def render_frame_run_disparity_baked_pool(layout, pool, frame0, nframes, homos, rows, H, W, spec: RenderSpec, out=None, *, quad_keep, culled_rgba8):
    """render_frame_run_disparity_baked from the baked POOL (vl3d_render_disp_baked_pool): `layout`, `pool`, `quad_keep`, `culled_rgba8` as
    render_frame_run_baked_pool takes them (a tap in a block without storage reads the alpha byte of culled_rgba8) -> the bits of
    render_frame_run_disparity_baked on the unpacked texels."""
    who = "render_frame_run_disparity_baked_pool"
    T, src = _baked_pool(who, layout, pool, homos, spec, quad_keep, culled_rgba8)
    _check_run(who, frame0, nframes, T, homos, src.dims[0], "model's")
    return _baked_disparity(who, src, int(nframes), frame0, None, homos, rows, H, W, spec, out)


def render_path_disparity_baked(baked, frame_cam, frame_t, homos, rows, H, W, spec: RenderSpec, quad_keep=None, out=None, cull_scratch=None):
    """The disparity maps of a camera path on the baked clip, one plan launch plus one render launch (vl3d_render_disp_baked with a path
    selection): output frame i is frame frame_t[i] seen by camera frame_cam[i] of `homos` [C,D,3,3] and `rows` [C,D,3]; the indices are
    range-checked here before they are uploaded (IndexError), as render_path_baked checks them.  -> (disp [N,H,W], alpha [N,H,W]) float32,
    frame i bit-equal to render_frame_run_disparity_baked(baked, frame_t[i], 1, homos[frame_cam[i]], rows[frame_cam[i]], ...)."""
    who = "render_path_disparity_baked"
    T, src = _baked_dense(who, baked, homos, spec, quad_keep)
    n, path = _check_path(who, frame_cam, frame_t, T, homos, src.dims[0], src.device)
    return _baked_disparity(who, src, n, 0, path, homos, rows, H, W, spec, out, cull_scratch)


def render_path_disparity_baked_pool(layout, pool, frame_cam, frame_t, homos, rows, H, W, spec: RenderSpec, out=None, *, quad_keep, culled_rgba8,
                                     cull_scratch=None):
    """render_path_disparity_baked from the baked POOL (vl3d_render_disp_baked_pool with a path selection)."""
    who = "render_path_disparity_baked_pool"
    T, src = _baked_pool(who, layout, pool, homos, spec, quad_keep, culled_rgba8)
    n, path = _check_path(who, frame_cam, frame_t, T, homos, src.dims[0], src.device)
    return _baked_disparity(who, src, n, 0, path, homos, rows, H, W, spec, out, cull_scratch)


# ---- RGB-D (include/vl3d.h "RGB-D"; csrc/vl3d_render_rgbd.hip) ----------------------------------------------------------------------------
def _rgbd_float_out(out, n, H, W, device, who):
    """(rgb [n,H,W,3], alpha [n,H,W], disp [n,H,W]) float32: fresh, or the caller's `out` triple checked."""
    if out is None:
        return _out_buffers(None, n, H, W, device, who) + (torch.empty((n, H, W), dtype=torch.float32, device=device),)
    if len(out) != 3:
        raise RuntimeError(f"{who}: `out` is (rgb [n,H,W,3], alpha [n,H,W], disp [n,H,W])")
    for b, shape in zip(out, ((n, H, W, 3), (n, H, W), (n, H, W))):
        if not isinstance(b, torch.Tensor) or b.device != device or b.dtype != torch.float32 or tuple(b.shape) != shape or not b.is_contiguous():
            raise RuntimeError(f"{who}: `out` must be contiguous float32 (rgb [n,H,W,3], alpha [n,H,W], disp [n,H,W]) with n,H,W = {n},{H},{W} "
                               "on the model's device")
    return tuple(out)


def _depth16_out(depth16, n, H, W, device, who):
    """the 16-bit depth of the display sink: uint16 [n,H,W] contiguous on `device`"""
    if (not isinstance(depth16, torch.Tensor) or depth16.device != device or depth16.dtype != torch.uint16 or tuple(depth16.shape) != (n, H, W)
            or not depth16.is_contiguous()):
        raise RuntimeError(f"{who}: `depth16` must be contiguous uint16 [n,H,W] = [{n},{H},{W}] on the model's device")
    return depth16


def _baked_rgbd(who, src, T, homos, rows, H, W, spec, run, path, times, out, frames8, depth16, bg, cull_scratch):
    """the one call of the two RGB-D renders: the selection (exactly one of run / path / times) checked by the colour wrappers' own checks, the
    sink (float triple, or frames8 with depth16) and the entry of the source `src` (_baked_dense / _baked_pool)"""
    if sum(v is not None for v in (run, path, times)) != 1:
        raise ValueError(f"{who}: exactly one of run=(frame0, n), path=(frame_cam, frame_t) and times=(frame_cam, frame_time)")
    if (frames8 is None) != (depth16 is None):
        raise ValueError(f"{who}: the display sink is `frames8=` AND `depth16=` (uint8 colour frames, uint16 depth): pass both or neither")
    _check_bg(who, frames8, bg)
    dev, D = src.device, src.dims[0]
    sel = tsel = None
    if run is not None:
        frame0, n = int(run[0]), int(run[1])
        _check_run(who, frame0, n, T, homos, D, "model's" if src.culled else "clip of")
        sel, n_cams = L.BakedFrames(frame0=frame0), None
    elif path is not None:
        n, (n_cams, idx) = _check_path(who, path[0], path[1], T, homos, D, dev)
        sel = L.BakedFrames(frame0=0, n_cams=n_cams, frame_cam=idx[0].data_ptr(), frame_t=idx[1].data_ptr())
    else:
        n, (n_cams, idx) = _check_times(who, times[0], times[1], T, homos, D, dev)
        tsel = L.BakedTimes(n_cams=n_cams, frame_cam=idx[0].data_ptr(), frame_time=idx[1].data_ptr())
    homos = homos.detach().to(torch.float32).contiguous()
    rows = _disp_rows(who, rows, homos, dev)
    desc = _desc_dims(D, n, src.dims[1], src.dims[2], H, W, spec, L.STACK_DTYPE["u8"])
    sink, entry = L.RgbdOut(), src.entry.replace("vl3d_render_fwd_", "vl3d_render_rgbd_")
    if frames8 is not None:
        sink.channels, bgc = _display_out(out, frames8, bg, n, H, W, dev, who)
        ret = (frames8, _depth16_out(depth16, n, H, W, dev, who))
        sink.frames, sink.bg, sink.depth16 = frames8.data_ptr(), (None if bgc is None else L.C.addressof(bgc)), depth16.data_ptr()
    else:
        ret = _rgbd_float_out(out, n, H, W, dev, who)
        sink.rgb, sink.alpha, sink.disp = (b.data_ptr() for b in ret)
    with torch.cuda.device(dev):
        cull = None
        if src.qk is not None:
            cull = _cull_scratch(desc, dev) if n_cams is None else _path_cull_scratch(desc, n_cams, dev, cull_scratch, who)
        grid = (0, 0) if src.qk is None else _qgrid(src.qk, spec)
        L.check(getattr(L.lib(), entry)(desc, *src.head, L.ptr(homos), L.ptr(rows), sel, tsel, L.ptr(src.qk), *grid, *src.culled, L.ptr(cull), sink,
                                        L.stream_ptr(dev)), entry)
    return ret


def render_rgbd_baked(baked, homos, rows, H, W, spec: RenderSpec, *, run=None, path=None, times=None, quad_keep=None, out=None, frames8=None,
                      depth16=None, bg=None, cull_scratch=None):
    """RGB-D frames of the baked clip in ONE render launch (vl3d_render_rgbd_baked): the picture of render_frame_run_baked / render_path_baked /
    render_times_baked and the disparity map of render_*_disparity_baked from one walk of the planes.  Exactly one selection, by keyword:
    `run` = (frame0, n) under homos [D,3,3] and rows [D,3]; `path` = (frame_cam, frame_t) or `times` = (frame_cam, frame_time) under homos
    [C,D,3,3] and rows [C,D,3] (depth_rows), checked as the colour wrappers check them.  -> (rgb [n,H,W,3], alpha [n,H,W], disp [n,H,W])
    float32 (`out`: the caller's triple): rgb and alpha bit-equal to the colour wrapper, disp of a run or a path to the disparity wrapper; a
    loop time has no other depth entry.  `frames8` (uint8 [n,H,W,3|4]) WITH `depth16` (uint16 [n,H,W]): the display sink instead -- the
    colour wrapper's display frames (over `bg`) and depth16 = trunc(65535 clip(disp, 0, 1)), not divided by alpha, 0 where nothing covers
    the pixel; normalise disp into [0, 1] through the rows (depth_rows(normalise=(near, far))).  -> (frames8, depth16).  Forward only."""
    who = "render_rgbd_baked"
    T, src = _baked_dense(who, baked, homos, spec, quad_keep)
    return _baked_rgbd(who, src, T, homos, rows, H, W, spec, run, path, times, out, frames8, depth16, bg, cull_scratch)


def render_rgbd_baked_pool(layout, pool, homos, rows, H, W, spec: RenderSpec, *, run=None, path=None, times=None, quad_keep, culled_rgba8, out=None,
                           frames8=None, depth16=None, bg=None, cull_scratch=None):
    """render_rgbd_baked from the baked POOL (vl3d_render_rgbd_baked_pool): `layout`, `pool`, `quad_keep`, `culled_rgba8` as
    render_frame_run_baked_pool takes them -> the bits of render_rgbd_baked on the unpacked texels."""
    who = "render_rgbd_baked_pool"
    T, src = _baked_pool(who, layout, pool, homos, spec, quad_keep, culled_rgba8)
    return _baked_rgbd(who, src, T, homos, rows, H, W, spec, run, path, times, out, frames8, depth16, bg, cull_scratch)


def render_planes(stack, homos, H, W, spec: RenderSpec = RenderSpec(), window=(0, 0), quad_keep=None, cull_window=None, grad_culled_unwritten=False,
                  fused_adam=None):
    """stack (D,T,Hs,Ws,4) pre-activation fp32 (plane 0 = nearest), homos [D,3,3] (target pixel -> plane pixel).

    Returns rgb [T,H,W,3], alpha [T,H,W].  `window=(row0,col0)` renders the H x W sub-window whose top-left
    corner is frame pixel (row0,col0) -- used for row-band sharding (equivalent to utils.py:196-200
    get_new_intrin on the target intrinsics).
    `quad_keep` [D,QH,QW] (bool/uint8, optional): tile culling map (videoloop3d_amd.tiles): a sample that falls into a culled quad
    of a plane is not covered by it, and workgroups skip the planes of which they see no kept quad (include/vl3d.h).
    `cull_window` (y0, x0, Hs_plane, Ws_plane), with quad_keep: `stack` is the texel window at (y0, x0) of a plane of that size and the
    quad grid lies over the whole plane (crop-aware training renders from a compact copy of the window, optim.WindowAdam).
    `grad_culled_unwritten` (with quad_keep): the consumer of the stack gradient never reads texels no kept quad can read (WindowAdam / TileAdam
    skip them), so the backward leaves those slots UNDEFINED instead of zero-filling them (VL3D_GRAD_CULLED_UNWRITTEN, include/vl3d.h).
    `fused_adam`: an optim.WindowAdam(fused_backward=True) whose pending window leaf `stack` is -- the backward then takes its step
    (vl3d_render_bwd_adam) and the leaf receives no gradient.
    This is the camera-differentiable entry: when `homos` requires a gradient the backward also returns d loss / d homos
    (vl3d_render_bwd_homos: float32 stacks, the planar and the utils_mpi convention, dense or a shared-border quad map, no cull_window, no
    fused step; anything else raises here).  The regulariser, loop-mask, view-dependent, plane-rows, packed and baked renders are not."""
    rgb, alpha, _, _ = _RenderPlanes.apply(stack, homos, int(H), int(W), spec, int(window[0]), int(window[1]), False, quad_keep, cull_window,
                                           bool(grad_culled_unwritten), fused_adam)
    return rgb, alpha


def _cam_system_args(who, stack, homos, dhomos, target, H, W, spec, window, quad_keep, weight, rgb, per_frame):
    """what render_normal_equations and render_register_equations check and prepare: -> (stack, homos, dhomos, target, weight, rgb, quad_keep,
    desc, P), contiguous float32 on the stack's device; `rgb` is the forward picture (rendered here if the caller gave none).  per_frame:
    target [T,H,W,3] and weight [T,H,W]; otherwise one picture, [H,W,3] and [H,W]."""
    L.check_cuda(stack, homos, dhomos, target)
    if spec.coord_mode == "affine_planes":
        raise RuntimeError(f"{who} is not built for per-plane records (coord_mode 'affine_planes')")
    if stack.dtype != torch.float32:
        raise RuntimeError(f"{who} is built for float32 stacks only, got {stack.dtype}")
    if getattr(spec, "tile", (0, 0))[0]:
        raise RuntimeError(f"{who} is not built for the tile-exact layout (RenderSpec.tile)")
    if getattr(spec, "uv_noise_seed", 0):
        raise RuntimeError(f"{who} is not built for add_uv_noise (uv_noise_seed = 0)")
    if int(spec.variant) != 0:
        raise RuntimeError(f"{who} has no kernel variants (spec.variant = 0)")
    conv = (spec.coord_mode, spec.border, spec.act_order)
    if conv not in (("affine", "hardcut", "post"), ("utils_mpi", "zeros", "pre")):
        raise RuntimeError(f"{who} is built for the planar convention (affine, hardcut, post) and the utils_mpi one (utils_mpi, zeros, pre), got {conv}")
    if stack.dim() != 5 or stack.shape[4] != 4:
        raise RuntimeError(f"{who}: the plane stack must be (D,T,Hs,Ws,4), got {tuple(stack.shape)}")
    D, T = int(stack.shape[0]), int(stack.shape[1])
    H, W = int(H), int(W)
    if T < 1 or H < 1 or W < 1:
        raise RuntimeError(f"{who}: nothing to fit on an empty picture (T = {T}, H = {H}, W = {W})")
    if tuple(homos.shape) != (D, 3, 3):
        raise RuntimeError(f"{who}: homos must be [D,3,3] = [{D},3,3], got {tuple(homos.shape)}")
    if dhomos.dim() != 4 or tuple(dhomos.shape[1:]) != (D, 3, 3) or not 1 <= dhomos.shape[0] <= 8:
        raise RuntimeError(f"{who}: dhomos must be [P,D,3,3] = [1..8,{D},3,3], got {tuple(dhomos.shape)}")
    frames, lead = ((T,), "T,") if per_frame else ((), "")
    dims = ",".join(str(v) for v in frames + (H, W))
    if tuple(target.shape) != frames + (H, W, 3):
        raise RuntimeError(f"{who}: target must be [{lead}H,W,3] = [{dims},3], got {tuple(target.shape)}")
    if weight is not None:
        L.check_cuda(weight)
        if tuple(weight.shape) != frames + (H, W):
            raise RuntimeError(f"{who}: weight must be [{lead}H,W] = [{dims}], got {tuple(weight.shape)}")
        weight = weight.detach().to(torch.float32).contiguous()
    if rgb is not None:
        L.check_cuda(rgb)
        if tuple(rgb.shape) != (T, H, W, 3):
            raise RuntimeError(f"{who}: rgb must be the forward picture [T,H,W,3] = [{T},{H},{W},3], got {tuple(rgb.shape)}")
    P = int(dhomos.shape[0])
    stack = stack.detach().contiguous()
    homos = homos.detach().to(torch.float32).contiguous()
    dhomos = dhomos.detach().to(torch.float32).contiguous()
    target = target.detach().to(torch.float32).contiguous()
    if quad_keep is not None:
        quad_keep = _quad_map(quad_keep, D)
    if rgb is None:
        with torch.no_grad():
            rgb, _ = render_planes(stack, homos, H, W, spec, window=window, quad_keep=quad_keep)
    rgb = rgb.detach().to(torch.float32).contiguous()
    desc = _desc(stack, H, W, spec, int(window[0]), int(window[1]))
    return stack, homos, dhomos, target, weight, rgb, quad_keep, desc, P


def render_normal_equations(stack, homos, dhomos, target, H, W, spec: RenderSpec = RenderSpec(), window=(0, 0), quad_keep=None, weight=None, rgb=None):
    """The Gauss-Newton system of the photometric residual rgb - target in P camera parameters (vl3d_render_cam_normal, include/vl3d.h
    "Camera normal equations"): stack (D,T,Hs,Ws,4) float32, homos [D,3,3], dhomos [P,D,3,3] = d homos / d theta_k (1 <= P <= 8;
    poses.camera_tangents), target [T,H,W,3], weight [T,H,W] or None (1), `window` and `quad_keep` as render_planes takes them.
    -> (A [P,P], b [P], cost) float64 tensors on the stack's device: A = sum w J^T J (symmetric), b = sum w J^T r, cost = sum w r^2 over
    frames, pixels and colour channels.  `rgb`: the forward picture [T,H,W,3] of the same arguments if the caller holds it; otherwise the
    existing forward runs here.  Not an autograd function: nothing it returns carries a graph.  It takes what the camera gradient takes
    (float32 stacks, the planar and the utils_mpi convention, dense or a shared-border quad map) and refuses the rest."""
    who = "render_normal_equations"
    stack, homos, dhomos, target, weight, rgb, quad_keep, desc, P = _cam_system_args(who, stack, homos, dhomos, target, H, W, spec, window, quad_keep,
                                                                                  weight, rgb, per_frame=True)
    out = torch.empty(P * P + P + 1, dtype=torch.float64, device=stack.device)
    with torch.cuda.device(stack.device):
        nb = int(L.lib().vl3d_render_cam_normal_scratch_bytes(desc, P))
        scratch = torch.empty((nb + 7) // 8, dtype=torch.float64, device=stack.device)
        L.check(L.lib().vl3d_render_cam_normal(desc, L.ptr(stack), L.ptr(homos), L.ptr(dhomos), P, *_qmap(quad_keep, spec), L.ptr(rgb), L.ptr(target),
                                               L.ptr(weight), L.ptr(out), L.ptr(scratch), nb, L.stream_ptr(stack.device)), "vl3d_render_cam_normal")
    return out[:P * P].view(P, P), out[P * P:P * P + P], out[P * P + P]


def render_register_equations(stack, homos, dhomos, target, H, W, spec: RenderSpec = RenderSpec(), window=(0, 0), quad_keep=None, weight=None, rgb=None,
                              long_exposure=False, brightness=None):
    """The Gauss-Newton system of registering a view against a CAPTURED clip (vl3d_render_cam_register, include/vl3d.h "Camera registration"):
    render_normal_equations with two additions.  `long_exposure`: the residual is taken on the temporal mean of the T rendered frames against
    ONE picture, target [H,W,3] (the clip's temporal mean; weight [H,W] or None) -- a clip of the same loop started at an unknown time has no
    frame-for-frame residual, its long exposure has one when it spans whole loop periods.  Otherwise target [T,H,W,3], weight [T,H,W].
    `brightness` = (log_gain, bias): the residual is exp(log_gain) picture + bias - target, and the log gain and the bias are two more unknowns
    after the P camera parameters, evaluated at that point; None: no brightness unknowns (gain 1, bias 0).
    -> (A [Q,Q], b [Q], cost) float64 on the stack's device, Q = P + 2 with `brightness`, else P.  Everything else -- stack, homos, dhomos,
    `window`, `quad_keep`, `rgb`, what is refused -- as render_normal_equations."""
    who = "render_register_equations"
    photo = brightness is not None
    log_gain, bias = (float(brightness[0]), float(brightness[1])) if photo else (0.0, 0.0)
    if not (math.isfinite(log_gain) and math.isfinite(bias)):
        raise RuntimeError(f"{who}: brightness = (log_gain, bias) must be finite, got {(log_gain, bias)}")
    stack, homos, dhomos, target, weight, rgb, quad_keep, desc, P = _cam_system_args(who, stack, homos, dhomos, target, H, W, spec, window, quad_keep,
                                                                                  weight, rgb, per_frame=not long_exposure)
    Q = P + 2 * int(photo)
    out = torch.empty(Q * Q + Q + 1, dtype=torch.float64, device=stack.device)
    with torch.cuda.device(stack.device):
        nb = int(L.lib().vl3d_render_cam_register_scratch_bytes(desc, P, int(photo)))
        scratch = torch.empty((nb + 7) // 8, dtype=torch.float64, device=stack.device)
        L.check(L.lib().vl3d_render_cam_register(desc, L.ptr(stack), L.ptr(homos), L.ptr(dhomos), P, *_qmap(quad_keep, spec), L.ptr(rgb), L.ptr(target),
                                                 L.ptr(weight), 1 if long_exposure else 0, int(photo), log_gain, bias, L.ptr(out), L.ptr(scratch), nb,
                                                 L.stream_ptr(stack.device)), "vl3d_render_cam_register")
    return out[:Q * Q].view(Q, Q), out[Q * Q:Q * Q + Q], out[Q * Q + Q]


def render_planes_with_smoothness(stack, homos, H, W, spec: RenderSpec = RenderSpec(), window=(0, 0), quad_keep=None):
    """render_planes plus the raw sums of the layer-space smoothness regularisers (MPV.py:517-531), differentiable:
    returns (rgb, alpha, sums[4]) with sums = (sum|dx rgb|, sum|dy rgb|, sum|dx a|, sum|dy a|) over frames, planes and
    neighbouring pixel pairs of the warped+activated layers -- the [T,h,w,K,4] layer tensor is never materialised."""
    rgb, alpha, sums, _ = _RenderPlanes.apply(stack, homos, int(H), int(W), spec, int(window[0]), int(window[1]), True, quad_keep)
    return rgb, alpha, sums


def render_planes_with_regularisers(stack, homos, H, W, spec: RenderSpec = RenderSpec(), window=(0, 0), quad_keep=None, cull_window=None,
                                    grad_culled_unwritten=False, fused_adam=None):
    """(rgb, alpha, smooth_sums[4], alpha_sums[T,H,W,2]): render_planes_with_smoothness plus the per-pixel (sum_k a_k,
    sum_k a_k^2) the sparsity regulariser |a|_1/|a|_2 (MPV.py:511-515, MPI.py:599-603) is built from; all differentiable."""
    return _RenderPlanes.apply(stack, homos, int(H), int(W), spec, int(window[0]), int(window[1]), True, quad_keep, cull_window,
                               bool(grad_culled_unwritten), fused_adam)


SH_C0, SH_C1 = 0.28209479177387814, 0.4886025119029199      # utils_mpi.py:321-322


def sh_ray_matrix(extrin, intrin):
    """The ray matrix of the view-dependent colour head (MPI.py:512-513 on utils.py:182-193): M = inverse(E)[:3,:3] inverse(K), E [4,4] (or
    [1,4,4]) the ref -> target extrinsic MPMesh.forward hands to render, K [3,3] the intrinsics of the call (the crop's) -> float32 [3,3] on
    the host, formed in float64.  Pixel (x, y) of the H x W image (integer indices, no half pixel) looks along d = normalize(M (x, y, 1)^T),
    in the reference camera's frame."""
    E = torch.as_tensor(extrin).detach().to("cpu", torch.float64).reshape(4, 4)
    K = torch.as_tensor(intrin).detach().to("cpu", torch.float64).reshape(3, 3)
    return (torch.linalg.inv(E)[:3, :3] @ torch.linalg.inv(K)).to(torch.float32)


def sh_basis(ray_m, H, W, window=(0, 0)):
    """the degree-1 basis b = (C0, -C1 d_y, C1 d_z, -C1 d_x) [H,W,4] of every pixel of the H x W window at frame pixel `window` = (row0, col0)
    (eval_sh_bases, utils_mpi.py:365-383, at the normalised rays of sh_ray_matrix), in torch on ray_m's device: the materialised-layer path and
    the tests read it; the render kernels form it themselves."""
    dev, dt = ray_m.device, ray_m.dtype
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=dt) + window[0], torch.arange(W, device=dev, dtype=dt) + window[1], indexing="ij")
    d = torch.stack([x, y, torch.ones_like(x)], -1) @ ray_m.T
    d = d / d.norm(dim=-1, keepdim=True)
    return torch.stack([torch.full_like(d[..., 0], SH_C0), -SH_C1 * d[..., 1], SH_C1 * d[..., 2], -SH_C1 * d[..., 0]], -1)


class _RenderPlanesSH(torch.autograd.Function):
    """render_planes with the view-dependent colour head (vl3d_render_sh_fwd / _bwd).  `homos` and `ray_m` get no gradient here:
    render_planes is the camera-differentiable entry."""

    @staticmethod
    def forward(ctx, stack, stack_sh, homos, ray_m, H, W, spec, row0, col0, quad_keep, with_alpha_sums):
        ctx.set_materialize_grads(False)
        L.check_cuda(stack, stack_sh, homos, ray_m)
        if stack.dim() != 5 or stack.shape[1] != 1 or stack.shape[4] != 4 or stack.dtype != torch.float32:
            raise RuntimeError(f"render_planes_sh: stack must be float32 (D,1,Hs,Ws,4), got {tuple(stack.shape)} {stack.dtype}")
        D, _, Hs, Ws, _ = stack.shape
        if tuple(stack_sh.shape) != (D, 1, Hs, Ws, 3, 4) or stack_sh.dtype != torch.float32 or stack_sh.device != stack.device:
            raise RuntimeError(f"render_planes_sh: stack_sh must be float32 (D,1,Hs,Ws,3,4) = {(D, 1, Hs, Ws, 3, 4)} on the stack's device, "
                               f"got {tuple(stack_sh.shape)} {stack_sh.dtype}")
        if tuple(homos.shape) != (D, 3, 3):
            raise RuntimeError(f"homos must be [D,3,3] = [{D},3,3], got {tuple(homos.shape)}")
        if tuple(ray_m.shape) != (3, 3):
            raise RuntimeError(f"ray_m must be [3,3] (render.sh_ray_matrix), got {tuple(ray_m.shape)}")
        if getattr(spec, "tile", (0, 0))[0]:
            raise RuntimeError("render_planes_sh: the tile-exact layout is not built for the view-dependent colour head")
        if quad_keep is not None:
            quad_keep = _quad_map(quad_keep, D)
        stack, stack_sh = stack.contiguous(), stack_sh.contiguous()
        homos = homos.detach().to(torch.float32).contiguous()
        ray_m = ray_m.detach().to(torch.float32).contiguous()
        rgb, alpha = _out_buffers(None, 1, H, W, stack.device, "render_planes_sh")
        asum = torch.empty((1, H, W, 2), dtype=torch.float32, device=stack.device) if with_alpha_sums else None
        ctx.nothing_to_render = H == 0 or W == 0
        if ctx.nothing_to_render:
            ctx.save_for_backward(stack, stack_sh)
            return rgb, alpha, (asum if with_alpha_sums else torch.zeros((0,), dtype=torch.float32, device=stack.device))
        desc = _desc(stack, H, W, spec, row0, col0)
        with torch.cuda.device(stack.device):
            L.check(L.lib().vl3d_render_sh_fwd(desc, L.ptr(stack), L.ptr(stack_sh), L.ptr(homos), L.ptr(ray_m), *_qmap(quad_keep, spec),
                                               L.ptr(rgb), L.ptr(alpha), L.ptr(asum), L.stream_ptr(stack.device)), "vl3d_render_sh_fwd")
        ctx.save_for_backward(stack, stack_sh, homos, ray_m, rgb, alpha)
        ctx.quad_keep, ctx.spec, ctx.desc, ctx.with_alpha_sums = quad_keep, spec, desc, with_alpha_sums
        return rgb, alpha, (asum if with_alpha_sums else torch.zeros((0,), dtype=torch.float32, device=stack.device))

    @staticmethod
    def backward(ctx, g_rgb, g_alpha, g_asum):
        if ctx.nothing_to_render:
            stack, stack_sh = ctx.saved_tensors
            return (torch.zeros_like(stack), torch.zeros_like(stack_sh)) + (None,) * 9
        stack, stack_sh, homos, ray_m, rgb, alpha = ctx.saved_tensors
        g_rgb = g_rgb.contiguous() if g_rgb is not None else torch.zeros_like(rgb)
        g_alpha = g_alpha.contiguous() if g_alpha is not None else None
        g_asum = g_asum.to(torch.float32).contiguous() if (ctx.with_alpha_sums and g_asum is not None) else None
        g_stack, g_sh = torch.empty_like(stack), torch.empty_like(stack_sh)      # (cleared by the entry: the sums are atomic)
        with torch.cuda.device(stack.device):
            L.check(L.lib().vl3d_render_sh_bwd(ctx.desc, L.ptr(stack), L.ptr(stack_sh), L.ptr(homos), L.ptr(ray_m), *_qmap(ctx.quad_keep, ctx.spec),
                                               L.ptr(rgb), L.ptr(alpha), L.ptr(g_rgb), L.ptr(g_alpha), L.ptr(g_asum), L.ptr(g_stack), L.ptr(g_sh),
                                               L.stream_ptr(stack.device)), "vl3d_render_sh_bwd")
        return (g_stack, g_sh) + (None,) * 9


def render_planes_sh(stack, stack_sh, homos, ray_m, H, W, spec: RenderSpec, quad_keep=None, with_alpha_sums=False, window=(0, 0)):
    """render_planes of a static MPI (T = 1) with the view-dependent colour head of stage 1 (rgb_mlp_type = "rgb_sh"; MPI.py:512-537,
    utils_mpi.py:50-61): stack (D,1,Hs,Ws,4) = (R0, G0, B0, alpha logit), stack_sh (D,1,Hs,Ws,3,4) with stack_sh[..., k - 1, c] the
    coefficient k = 1..3 of colour c (lane 3 reserved: 0), homos [D,3,3], ray_m [3,3] on the device (sh_ray_matrix).  Per pixel the colour
    logits are sum_k b_k sample(coef_k) with the degree-1 basis b of the pixel's normalised ray; everything else as render_planes in the
    planar convention (RenderSpec.mpv(...), any activation pair, fp32).  `quad_keep` [D,QH,QW]: a tile-culled model (shared borders).
    -> (rgb [1,H,W,3], alpha [1,H,W]) or, with_alpha_sums, (rgb, alpha, alpha_sums [1,H,W,2]).  Differentiable w.r.t. both stacks; the
    gradient is summed with float atomics and is not bit-reproducible between runs; lane 3 of stack_sh's gradient is exactly 0."""
    rgb, alpha, asum = _RenderPlanesSH.apply(stack, stack_sh, homos, ray_m, int(H), int(W), spec, int(window[0]), int(window[1]), quad_keep,
                                             bool(with_alpha_sums))
    return (rgb, alpha, asum) if with_alpha_sums else (rgb, alpha)


class _RenderPlaneRows(torch.autograd.Function):
    """render_planes of a row band from PER-PLANE local rows (vl3d_render_fwd_plane_rows / _bwd_plane_rows): local row r of plane d is
    plane row plane_row0[d] + r; the gradient comes back in the same local layout, padding rows 0.  `homos` gets no gradient here:
    render_planes is the camera-differentiable entry."""

    @staticmethod
    def forward(ctx, local, homos, plane_row0, H, W, Hs, spec, row0, col0):
        L.check_cuda(local, homos, plane_row0)
        if local.dtype not in (torch.float32, torch.float16) or local.dim() != 5 or local.shape[4] != 4:
            raise RuntimeError("per-plane local stack must be float32 / float16 (D,T,R,Ws,4)")
        D, T, R = local.shape[:3]
        if homos.shape != (D, 3, 3):
            raise RuntimeError(f"homos must be [D,3,3] = [{D},3,3], got {tuple(homos.shape)}")
        if plane_row0.dtype != torch.int32 or tuple(plane_row0.shape) != (D,) or plane_row0.device != local.device:
            raise RuntimeError(f"plane_row0 must be an int32 [D] = [{D}] tensor on the stack's device")
        local = local.contiguous()
        homos = homos.detach().to(torch.float32).contiguous()
        plane_row0 = plane_row0.contiguous()
        desc = _desc(local, H, W, spec, row0, col0)
        desc.Hs = int(Hs)             # the TRUE plane height: coverage / hard cut (the stack holds R rows per plane)
        rgb = torch.empty((T, H, W, 3), dtype=torch.float32, device=local.device)
        alpha = torch.empty((T, H, W), dtype=torch.float32, device=local.device)
        with torch.cuda.device(local.device):
            L.check(L.lib().vl3d_render_fwd_plane_rows(desc, L.ptr(local), L.ptr(plane_row0), int(R), L.ptr(homos), L.ptr(rgb), L.ptr(alpha),
                                                       L.stream_ptr(local.device)), "vl3d_render_fwd_plane_rows")
        ctx.save_for_backward(local, homos, plane_row0, rgb, alpha)
        ctx.desc, ctx.R = desc, int(R)
        return rgb, alpha

    @staticmethod
    def backward(ctx, g_rgb, g_alpha):
        local, homos, plane_row0, rgb, alpha = ctx.saved_tensors
        dev = local.device
        g_rgb = g_rgb.contiguous() if g_rgb is not None else torch.zeros_like(rgb)
        g_alpha = g_alpha.contiguous() if g_alpha is not None else None
        g_local = torch.empty(local.shape, dtype=local.dtype, device=dev)
        with torch.cuda.device(dev):
            nscratch = int(L.lib().vl3d_render_plane_rows_scratch_bytes(ctx.desc, ctx.R))
            # plan, tile windows and owner table of the owner-computes backward: every word read is written by the same call
            scratch = torch.empty((nscratch + 3) // 4, dtype=torch.float32, device=dev)
            L.check(L.lib().vl3d_render_bwd_plane_rows(ctx.desc, L.ptr(local), L.ptr(plane_row0), ctx.R, L.ptr(homos), L.ptr(rgb), L.ptr(alpha),
                                                       L.ptr(g_rgb), L.ptr(g_alpha), L.ptr(g_local), L.ptr(scratch), nscratch, L.stream_ptr(dev)),
                    "vl3d_render_bwd_plane_rows")
        global LAST_BWD_SCRATCH, LAST_BWD_CALL
        LAST_BWD_SCRATCH, LAST_BWD_CALL = scratch, None      # (its own frame-pair launch: vl3d_render_bwd_choice does not describe it)
        return g_local, None, None, None, None, None, None, None, None


def render_plane_rows(local, homos, plane_row0, H, W, Hs, spec: RenderSpec, window=(0, 0)):
    """The H x W window at frame pixel `window` = (row0, col0) rendered from per-plane local rows: local (D,T,R,Ws,4), plane d's local row r
    being its plane row plane_row0[d] + r (plane_row0: int32 [D] on the device), Hs the true plane height.  The same bits as
    render_planes(full_stack, ..., window=window) wherever the windows hold every row the band's taps reach (dist.plan_plane_bands).
    The planar MPV convention (RenderSpec.mpv(), sigmoid / sigmoid), fp32 or fp16 stacks.  -> (rgb [T,H,W,3], alpha [T,H,W])."""
    if spec.act_order == "baked":
        raise RuntimeError("per-plane row windows are not built for the bake rule (act_order='baked'): render the band from the whole stack (render_planes)")
    if spec.coord_mode != "affine" or spec.border != "hardcut" or spec.act_order != "post":
        raise RuntimeError("per-plane row windows render in the planar MPV convention (RenderSpec.mpv())")
    return _RenderPlaneRows.apply(local, homos, plane_row0, int(H), int(W), int(Hs), spec, int(window[0]), int(window[1]))


@torch.no_grad()
def render_planes_packed(layout, pool, frames, homos, H, W, spec: RenderSpec, quad_keep, culled_alpha, out=None, frames_dev=None):
    """The forward of a PACKED tile-culled model straight from its pool (videoloop3d_amd/packed.py; the reference renders a sparsified model
    from its tile lists, MPV.py:389-449): rgb [n,H,W,3], alpha [n,H,W] for the chosen `frames` -- the bits of the culled render of the
    unpacked frames, without ever building them.  No gradient (evaluation renders; training goes through the optimiser's window copy;
    render_planes is the camera-differentiable entry).
    `out`: (rgb, alpha) buffers to write into; `frames_dev`: the same frame indices as an int32 device tensor (a caller rendering a long path
    uploads them once instead of per call)."""
    L.check_cuda(pool, homos, quad_keep, layout.blocks)
    if spec.act_order == "baked":
        raise RuntimeError("a packed model is not rendered under the bake rule (act_order='baked'): baked.bake_pool(model) gives its playback model")
    if spec.coord_mode != "affine" or spec.border != "hardcut" or spec.act_order != "post":
        raise RuntimeError("a packed model renders in the planar MPV convention (RenderSpec.mpv())")
    frames = [int(t) for t in frames]
    if not frames:
        return (torch.empty((0, H, W, 3), dtype=torch.float32, device=pool.device), torch.empty((0, H, W), dtype=torch.float32, device=pool.device))
    if min(frames) < 0 or max(frames) >= layout.T:
        raise IndexError(f"frame index out of range [0, {layout.T})")
    homos = homos.detach().to(torch.float32).contiguous()
    if homos.shape != (layout.D, 3, 3):
        raise RuntimeError(f"homos must be [D,3,3] = [{layout.D},3,3], got {tuple(homos.shape)}")
    d = _desc_dims(layout.D, layout.T, layout.Hs, layout.Ws, H, W, spec)      # (the planar convention: checked above)
    d.variant, d.uv_noise_seed = 0, 0
    dev = pool.device
    qk = _quad_map(quad_keep, layout.D)
    if frames_dev is not None:
        if frames_dev.dtype != torch.int32 or frames_dev.numel() != len(frames) or not frames_dev.is_contiguous() or frames_dev.device != dev:
            raise RuntimeError("render_planes_packed: frames_dev must be the contiguous int32 device copy of `frames`")
        ft = frames_dev
    else:
        ft = torch.tensor(frames, dtype=torch.int32).to(dev, non_blocking=True)
    rgb, alpha = _out_buffers(out, len(frames), H, W, dev, "render_planes_packed")
    with torch.cuda.device(dev):
        L.check(L.lib().vl3d_render_fwd_packed(d, L.ptr(layout.blocks), L.ptr(pool), L.ptr(ft), len(frames), L.ptr(homos), L.ptr(qk), *_qgrid(qk, spec), float(culled_alpha), L.ptr(rgb), L.ptr(alpha), L.stream_ptr(dev)), "vl3d_render_fwd_packed")
    return rgb, alpha
