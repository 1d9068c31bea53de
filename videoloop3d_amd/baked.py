"""The playback model: what ships, baked to RGBA8 on the device, rendered the way a player shows it.

The reference's viewer package (scripts/script_export_mesh.py:117-191: geometry.obj, static.png, dynamic/%04d.png, meta.json) holds the
atlases ACTIVATED, multiplied by 255, clipped and truncated to 8 bits; a player filters those texels bilinearly, after the activation.
`MPMeshVid.forward` interpolates fp32 texels first and activates afterwards -- a different picture.

  bake_texels(t, rgb_act, alpha_act)   the ONE bake rule, u8 = uint8(trunc(clip(act(s) * 255, 0, 255))) per channel (straight RGBA):
                                       vl3d_bake_rgba8 for device tensors, the same expression in torch for host tensors (the export runs there).
  bake(module) -> BakedMPV             the uint8 texels (D,T,Hs,Ws,4) of an MPMeshVid with its quad map, render geometry, background and
                                       camera: renders without the float stack (render.render_frame_run_baked), a quarter of its bytes.
"""
import torch

from . import _lib as L
from .plane_model import ACTIVATES, PlaneModel


def bake_texels(t, rgb_act, alpha_act):
    """[...,4] float32 / float16 pre-activation rgba texels -> uint8 of the same shape: channels 0-2 through `rgb_act`, channel 3 through
    `alpha_act` (names of the activation table), times 255, clipped to [0, 255], TRUNCATED (script_export_mesh.py:130-138)."""
    if rgb_act not in ACTIVATES or alpha_act not in ACTIVATES:
        raise RuntimeError(f"activation ({rgb_act}, {alpha_act}) not in the activation table {sorted(ACTIVATES)}")
    if t.shape[-1] != 4 or t.dtype not in (torch.float32, torch.float16):
        raise RuntimeError(f"bake_texels: float32 / float16 rgba texels [...,4], got {tuple(t.shape)} {t.dtype}")
    t = t.detach()
    if not t.is_cuda:
        s = t.float()
        a = torch.cat([ACTIVATES[rgb_act](s[..., :3]), ACTIVATES[alpha_act](s[..., 3:])], dim=-1)
        return (a * 255).clamp(0, 255).to(torch.uint8)
    t = t.contiguous()
    out = torch.empty(t.shape, dtype=torch.uint8, device=t.device)
    if t.numel() == 0:
        return out
    with torch.cuda.device(t.device):
        L.check(L.lib().vl3d_bake_rgba8(t.numel() // 4, L.ptr(t), L.STACK_DTYPE["f16" if t.dtype == torch.float16 else "f32"], L.ACT[rgb_act],
                                        L.ACT[alpha_act], L.ptr(out), L.stream_ptr(t.device)), "vl3d_bake_rgba8")
    return out


class _Camera:
    """the camera side of a plane model without its texture: reference camera, plane depths and the module's own `plane_homographies`
    (the same code object: the same bits as the module's forward)."""
    plane_homographies = PlaneModel.plane_homographies
    _host_np = PlaneModel._host_np
    _on = PlaneModel._on

    def __init__(self, module):
        self.args, self.mpi_d = module.args, module.mpi_d
        for name in ("ref_extrin", "ref_intrin_mpi", "planedepth"):
            setattr(self, name, getattr(module, name).detach().clone())


class BakedMPV:
    """bake(module)'s product.  texels [D,T,Hs,Ws,4] uint8 on the device, quad_keep [D,QH,QW] uint8 or None, spec (render.RenderSpec: pixel
    centre, texel scale / offset, tile-exact layout), bg_color, camera (plane_homographies, ref_extrin)."""

    def __init__(self, texels, quad_keep, spec, bg_color, camera):
        self.texels, self.quad_keep, self.spec, self.bg_color, self.camera = texels, quad_keep, spec, bg_color, camera

    @property
    def nbytes(self):
        """bytes of the baked texels: a quarter of the fp32 stack's."""
        return self.texels.numel() * self.texels.element_size()

    @property
    def frm_num(self):
        return int(self.texels.shape[1])

    def extrins_to_ref(self, tar_extrins):
        """world-to-camera poses -> reference-camera-to-target transforms, as MPMeshVid.forward forms them (MPV.py:481)."""
        return tar_extrins @ self.camera._on(tar_extrins.device, "ref_extrin")[None, ...].inverse().to(tar_extrins.dtype)

    def background(self):
        """the background colour of this call as a device tensor, or None (MPV.py:455-461: "" none, "random" one draw per call, "r#g#b")."""
        if len(self.bg_color) == 0:
            return None
        if self.bg_color == "random":
            return torch.rand(3).to(self.texels.device)
        return torch.tensor([float(v) for v in self.bg_color.split('#')], dtype=torch.float32, device=self.texels.device)

    @torch.no_grad()
    def render(self, H, W, extrins, intrins, ts=None):
        """the module's eval forward on the baked texels: one camera (extrins [1,4,4] world-to-camera, intrins [1,3,3]), frames `ts` (default:
        the whole clip) -> (rgb [T',3,H,W] over the background, alpha [T',H,W])."""
        from .render import render_frame_run_baked
        extrins, intrins = torch.as_tensor(extrins), torch.as_tensor(intrins)
        tl = list(range(self.frm_num)) if ts is None else [int(t) for t in torch.as_tensor(ts).reshape(-1).tolist()]
        dev = self.texels.device
        homos = self.camera.plane_homographies(self.extrins_to_ref(extrins), intrins).to(dev)
        rgb = torch.empty((len(tl), H, W, 3), dtype=torch.float32, device=dev)
        alpha = torch.empty((len(tl), H, W), dtype=torch.float32, device=dev)
        i = 0
        while i < len(tl):      # runs of consecutive frames are read where they lie in the clip
            j = i + 1
            while j < len(tl) and tl[j] == tl[j - 1] + 1:
                j += 1
            if not (0 <= tl[i] and tl[j - 1] < self.frm_num):
                raise IndexError(f"frame index {tl[i]} .. {tl[j - 1]} outside the clip of {self.frm_num} frames")
            render_frame_run_baked(self.texels, tl[i], j - i, homos, H, W, self.spec, out=(rgb[i:j], alpha[i:j]), quad_keep=self.quad_keep)
            i = j
        bg = self.background()
        if bg is not None:
            rgb = rgb * alpha[..., None] + bg[None, None, None] * (-alpha[..., None] + 1)
        return rgb.permute(0, 3, 1, 2), alpha


@torch.no_grad()
def bake(module):
    """MPMeshVid (dense, or sparsified in either tile layout) -> BakedMPV.  A packed model, an `atlas_exact` model and a model on the host are
    refused: the baked render reads a dense uint8 stack in the planar convention, on the device."""
    module = getattr(module, "module", module)
    if getattr(module, "packed", None) is not None:
        raise RuntimeError("bake: a packed model has no dense stack to bake (bake before pack_(), or load the checkpoint with packed=False)")
    if getattr(module, "atlas_exact", False):
        raise RuntimeError("bake: atlas_exact models sample the reference's atlas cells; the baked render is built for the planar convention")
    stack = getattr(module, "stack", None)
    if stack is None or stack.dim() != 5 or not hasattr(module, "frm_num"):
        raise RuntimeError("bake: an MPMeshVid with its dense (D,T,Hs,Ws,4) stack")
    if not stack.is_cuda:
        raise RuntimeError("bake: the model is on the host; the baked model lives and renders on the device (module.cuda() first)")
    module._flush_deferred_updates()
    texels = bake_texels(module.stack.data, module.args.rgb_activate, module.args.alpha_activate)
    qk = None
    if module.is_sparse and getattr(module, "quad_keep", None) is not None:
        qk = module.quad_keep.to(torch.uint8).contiguous().clone()
    return BakedMPV(texels, qk, module.spec, str(module.args.bg_color), _Camera(module))
