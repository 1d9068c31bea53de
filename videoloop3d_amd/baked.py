"""The playback model: what ships, baked to RGBA8 on the device, rendered the way a player shows it.

The reference's viewer package (scripts/script_export_mesh.py:117-191: geometry.obj, static.png, dynamic/%04d.png, meta.json) holds the
atlases ACTIVATED, multiplied by 255, clipped and truncated to 8 bits; a player filters those texels bilinearly, after the activation.
`MPMeshVid.forward` interpolates fp32 texels first and activates afterwards -- a different picture.

  bake_texels(t, rgb_act, alpha_act)   the ONE bake rule, u8 = uint8(trunc(clip(act(s) * 255, 0, 255))) per channel (straight RGBA):
                                       vl3d_bake_rgba8 for device tensors, the same expression in torch for host tensors (the export runs there).
  bake(module) -> BakedMPV             the uint8 texels (D,T,Hs,Ws,4) of an MPMeshVid with its quad map, render geometry, background and
                                       camera: renders without the float stack (render.render_frame_run_baked), a quarter of its bytes.
  bake_pool(module) -> BakedPool       the same for a tile-culled model, packed or not, WITHOUT a dense clip: RGBA8 blocks of 8 x 8 texels behind the
                                       block table of packed.PackedLayout (static blocks once, dynamic blocks per frame, culled blocks not at all --
                                       the static and the dynamic atlas of the viewer package), rendered by render.render_frame_run_baked_pool with
                                       the bits of the dense baked render.  256 bytes per slot: a quarter of the float pool.
  display_frames(rgb, alpha, bg, C)    the ONE display rule: a float render -> the uint8 frames a viewer shows (over the background, to8b).
  BakedMPV / BakedPool.render_display  poses in, uint8 frames out: the render kernels store that rule's bytes themselves (`frames8=`).
  BakedPool.trimmed()                  the pool without what a player provably cannot show: blocks that never show dropped, frozen dynamic blocks
                                       stored once, quads of alpha byte 0 off the map -- every frame keeps its bits (vl3d_baked_trim_*).
  loop_times(times, T)                 any real playback times -> float32 loop times in [0, T): what `fractional=True` of render_path /
                                       render_display renders, texels interpolated between adjacent frames and across the loop seam.
"""
import copy

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


def display_frames(rgb, alpha, bg=None, channels=3):
    """The display rule in torch: rgb [N,H,W,3], alpha [N,H,W] float32 -> uint8 [N,H,W,channels].  Over `bg` (3 floats or a tensor of 3, or
    None) as MPV.py:455-461 composites, then to8b (utils.py: (255 * clip(x, 0, 1)).astype(uint8), truncating); channels == 4 appends the alpha
    byte, to8b of alpha itself, never composited.  The `frames8=` sink of the baked renders (the display sink of vl3d_render_fwd_baked / _pool) stores these bytes."""
    if channels not in (3, 4):
        raise ValueError(f"display_frames: channels must be 3 (RGB8) or 4 (RGBA8), got {channels}")
    x = rgb
    if bg is not None:
        bg = torch.as_tensor(bg, dtype=torch.float32).to(rgb.device)
        x = rgb * alpha[..., None] + bg[None, None, None] * (-alpha[..., None] + 1)
    out = (255 * x.clamp(0, 1)).to(torch.uint8)
    if channels == 4:
        out = torch.cat([out, (255 * alpha.clamp(0, 1)).to(torch.uint8)[..., None]], dim=-1)
    return out


def loop_times(times, T):
    """Real playback times, of any sign and size -> float32 numpy array of loop times in [0, T), the `frame_time` of render.render_times_baked /
    _pool.  The loop has T frames and frame T is frame 0 again: the reduction is t - T floor(t / T) in float64 (negative times wrap:
    -0.25 -> T - 0.25), then the cast to float32; a value the cast (or the float64 subtraction) rounds up to T -- -1e-9 -- is 0.0, the same
    instant of the loop.  A non-finite time is a ValueError."""
    import numpy as np
    T = int(T)
    if T < 1:
        raise ValueError(f"loop_times: a loop of T >= 1 frames, got {T}")
    t = np.asarray(times, dtype=np.float64).reshape(-1)
    if not np.isfinite(t).all():
        raise ValueError("loop_times: a time is not finite")
    r = (t - T * np.floor(t / T)).astype(np.float32)
    r[~((r >= 0) & (r < T))] = 0.0      # T itself (rounded up), or -0.0 / a last-bit negative of the subtraction
    return r


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

    def depth_rows(self, extrins_to_ref, intrins, normalise=None):
        """the affine rows of the planes' inverse view depth (render.depth_rows) under ref -> target extrinsics [C,4,4] / intrinsics [C,3,3];
        `normalise` = (near, far): folded into the rows"""
        from .render import depth_rows
        return depth_rows(extrins_to_ref, intrins, self.planedepth, normalise)


def path_cameras(camera, view_extrins, view_intrins):
    """the DISTINCT cameras of a path: (view_extrins [N,4,4] world-to-camera, view_intrins [N,3,3], host float tensors) -> (cam_of: for every
    pose the index of its camera, in order of first appearance; homos [C,D,3,3] on the host: `camera.plane_homographies` of each distinct
    camera -- the module's own code object, called pose by pose: the bits of its forward).  Poses are equal when their bytes are."""
    ref_inv = camera._on(view_extrins.device, "ref_extrin")[None, ...].inverse().to(view_extrins.dtype)
    cams, cam_of = {}, []
    for i in range(len(view_extrins)):
        key = (view_extrins[i].numpy().tobytes(), view_intrins[i].numpy().tobytes())
        if key not in cams:
            cams[key] = (len(cams), camera.plane_homographies(view_extrins[i:i + 1] @ ref_inv, view_intrins[i:i + 1]))
        cam_of.append(cams[key][0])
    return cam_of, torch.stack([h for _, h in sorted(cams.values(), key=lambda c: c[0])])


class _Baked:
    """what BakedMPV and BakedPool share: camera, background and the module's eval forward over runs of consecutive frames.  A subclass has
    `device`, `frm_num`, `bg_color`, `camera`, `_run(frame0, n, homos, H, W, out)`: its render of a run of frames, read in place, and
    `_path(frame_cam, frame_t, homos [C,D,3,3], H, W, out)`: its render of a camera path; both take `frames8=`, `bg=` for the display frames.
    `_times(frame_cam, frame_time, homos, H, W, out)`: the path in loop time (`fractional=True`), float32 times in [0, frm_num).
    `_rgbd(homos, rows, H, W, run= | path= | times=, out= | frames8=, depth16=, bg=)`: its RGB-D render (render.render_rgbd_baked / _pool)."""

    def extrins_to_ref(self, tar_extrins):
        """world-to-camera poses -> reference-camera-to-target transforms, as MPMeshVid.forward forms them (MPV.py:481)."""
        return tar_extrins @ self.camera._on(tar_extrins.device, "ref_extrin")[None, ...].inverse().to(tar_extrins.dtype)

    def background(self):
        """the background colour of this call as a device tensor, or None (MPV.py:455-461: "" none, "random" one draw per call, "r#g#b")."""
        if len(self.bg_color) == 0:
            return None
        if self.bg_color == "random":
            return torch.rand(3).to(self.device)
        return torch.tensor([float(v) for v in self.bg_color.split('#')], dtype=torch.float32, device=self.device)

    @torch.no_grad()
    def render(self, H, W, extrins, intrins, ts=None):
        """the module's eval forward on the baked texels: one camera (extrins [1,4,4] world-to-camera, intrins [1,3,3]), frames `ts` (default:
        the whole clip) -> (rgb [T',3,H,W] over the background, alpha [T',H,W])."""
        extrins, intrins = torch.as_tensor(extrins), torch.as_tensor(intrins)
        tl = list(range(self.frm_num)) if ts is None else [int(t) for t in torch.as_tensor(ts).reshape(-1).tolist()]
        dev = self.device
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
            self._run(tl[i], j - i, homos, H, W, (rgb[i:j], alpha[i:j]))
            i = j
        bg = self.background()
        if bg is not None:
            rgb = rgb * alpha[..., None] + bg[None, None, None] * (-alpha[..., None] + 1)
        return rgb.permute(0, 3, 1, 2), alpha


    @torch.no_grad()
    def render_path(self, H, W, extrins, intrins, ts, fractional=False):
        """a camera path in one plan launch plus one render launch (render.render_path_baked / _pool): N poses (extrins [N,4,4] world-to-camera,
        intrins [N,3,3]), output frame i showing frame ts[i] of the clip -> (rgb [N,3,H,W] over the background, alpha [N,H,W]); frame i has
        the bits of render(H, W, extrins[i:i+1], intrins[i:i+1], ts[i:i+1]).  `fractional`: ts are real LOOP TIMES of any sign and size
        (loop_times reduces them into the loop): the texels are interpolated between the two adjacent frames, the last and the first
        included (render.render_times_baked / _pool); without it every entry of ts is truncated to a frame index."""
        extrins = torch.as_tensor(extrins, dtype=torch.float32).cpu()
        intrins = torch.as_tensor(intrins, dtype=torch.float32).cpu()
        if fractional:
            tl = loop_times(torch.as_tensor(ts).reshape(-1).tolist(), self.frm_num)
        else:
            tl = [int(t) for t in torch.as_tensor(ts).reshape(-1).tolist()]
        if not (len(extrins) == len(intrins) == len(tl)):
            raise RuntimeError(f"render_path: one pose and one frame per output frame ({len(extrins)} extrins, {len(intrins)} intrins, {len(tl)} frames)")
        cam_of, homos = path_cameras(self.camera, extrins, intrins)
        rgb, alpha = (self._times if fractional else self._path)(cam_of, tl, homos.pin_memory().to(self.device, non_blocking=True), H, W, None)
        bg = self.background()
        if bg is not None:
            rgb = rgb * alpha[..., None] + bg[None, None, None] * (-alpha[..., None] + 1)
        return rgb.permute(0, 3, 1, 2), alpha

    @torch.no_grad()
    def render_disparity(self, H, W, extrins, intrins, ts, max_batch=64):
        """The depth maps of a camera path on the baked texels (render.render_path_disparity_baked / _pool; include/vl3d.h "Disparity"): N poses
        (extrins [N,4,4] world-to-camera, intrins [N,3,3]), output frame i showing frame ts[i] -> (disp [N,H,W], alpha [N,H,W]) float32 on the
        device: per pixel the colour composite's own blend weights (alpha has the bits of render_path's) times the inverse view depth of every
        plane.  Equal poses share a camera (path_cameras); chunks of at most `max_batch` frames go as render_video.path_segments says -- a
        chunk that is one run as one run call, any other as one path call -- with the same bits either way."""
        from .render_video import path_segments
        extrins = torch.as_tensor(extrins, dtype=torch.float32).cpu()
        intrins = torch.as_tensor(intrins, dtype=torch.float32).cpu()
        tl = [int(t) for t in torch.as_tensor(ts).reshape(-1).tolist()]
        n, dev = len(tl), self.device
        if not (len(extrins) == len(intrins) == n):
            raise RuntimeError(f"render_disparity: one pose and one frame per output frame ({len(extrins)} extrins, {len(intrins)} intrins, {n} frames)")
        disp = torch.empty((n, H, W), dtype=torch.float32, device=dev)
        alpha = torch.empty((n, H, W), dtype=torch.float32, device=dev)
        if n == 0:
            return disp, alpha
        cam_of, homos = path_cameras(self.camera, extrins, intrins)
        first = [cam_of.index(c) for c in range(len(homos))]      # a pose of every distinct camera
        rows = self.camera.depth_rows(self.extrins_to_ref(extrins[first]), intrins[first])
        both = torch.cat([homos.to(torch.float32).reshape(-1), rows.reshape(-1)])      # homographies and rows of every camera: one pinned copy
        if dev.type == "cuda":
            both = both.pin_memory().to(dev, non_blocking=True)
        homos, rows = both[:homos.numel()].view(homos.shape), both[homos.numel():].view(rows.shape)
        for kind, c0, c1 in path_segments(cam_of, tl, max_batch):
            out = (disp[c0:c1], alpha[c0:c1])
            if kind == "run":
                if not (0 <= tl[c0] and tl[c1 - 1] < self.frm_num):
                    raise IndexError(f"frame index {tl[c0]} .. {tl[c1 - 1]} outside the clip of {self.frm_num} frames")
                self._disparity_run(tl[c0], c1 - c0, homos[cam_of[c0]], rows[cam_of[c0]], H, W, out)
            else:
                lo, hi = min(cam_of[c0:c1]), max(cam_of[c0:c1]) + 1      # the chunk's cameras: a slice of the path's
                self._disparity_path([c - lo for c in cam_of[c0:c1]], tl[c0:c1], homos[lo:hi], rows[lo:hi], H, W, out)
        return disp, alpha

    @torch.no_grad()
    def render_rgbd(self, H, W, extrins, intrins, ts, fractional=False, normalise=True, display=False, channels=3, out=None, max_batch=64):
        """RGB-D frames of a camera path, colour and depth from ONE render launch per chunk (render.render_rgbd_baked / _pool; include/vl3d.h
        "RGB-D"): N poses (extrins [N,4,4] world-to-camera, intrins [N,3,3]), output frame i showing frame ts[i] of the clip -- or, with
        `fractional`, the model at the real loop time ts[i] (loop_times reduces it), which no other depth entry renders.
        -> (rgb [N,H,W,3], alpha [N,H,W], disp [N,H,W]) float32 on the device: rgb and alpha with the bits of render_path before its
        background, disp with the bits of render_disparity under the same rows; or, with `display`, (frames8 uint8 [N,H,W,channels], depth16
        uint16 [N,H,W]): render_display's bytes and trunc(65535 clip(disp, 0, 1)), not divided by alpha, 0 where no plane covers the pixel.
        `normalise`: True maps the inverse depth of the nearest plane to 1 and of the farthest to 0 (folded into the rows,
        render.depth_rows(normalise=(near, far))), a (near, far) pair names the range, False leaves the inverse view depth as it is
        (render_disparity's).  `out`: the caller's triple or pair, written in place.  Chunks of at most `max_batch` frames go as
        render_video.path_segments says -- one run call or one path call, the same bits either way; every chunk of loop times is one call."""
        from .render_video import path_segments
        extrins = torch.as_tensor(extrins, dtype=torch.float32).cpu()
        intrins = torch.as_tensor(intrins, dtype=torch.float32).cpu()
        if fractional:
            tl = loop_times(torch.as_tensor(ts).reshape(-1).tolist(), self.frm_num)
        else:
            tl = [int(t) for t in torch.as_tensor(ts).reshape(-1).tolist()]
        n, dev = len(tl), self.device
        if not (len(extrins) == len(intrins) == n):
            raise RuntimeError(f"render_rgbd: one pose and one frame per output frame ({len(extrins)} extrins, {len(intrins)} intrins, {n} frames)")
        if display:
            if channels not in (3, 4):
                raise ValueError(f"render_rgbd: channels must be 3 (RGB8) or 4 (RGBA8), got {channels}")
            bg = self.display_bg()
            shapes = (((n, H, W, channels), torch.uint8), ((n, H, W), torch.uint16))
        else:
            bg = None
            shapes = (((n, H, W, 3), torch.float32), ((n, H, W), torch.float32), ((n, H, W), torch.float32))
        if out is None:
            out = tuple(torch.empty(s, dtype=d, device=dev) for s, d in shapes)
        elif len(out) != len(shapes) or any(b.dtype != d or tuple(b.shape) != s or not b.is_contiguous() or b.device != dev
                                           for b, (s, d) in zip(out, shapes)):
            raise RuntimeError(f"render_rgbd: `out` must be contiguous tensors {[(s, str(d)) for s, d in shapes]} on the model's device")
        if n == 0:
            return tuple(out)
        if normalise is True:
            z = self.camera.planedepth.detach().double().reshape(-1)
            normalise = (float(z.min()), float(z.max()))
        elif normalise is False:
            normalise = None
        cam_of, homos = path_cameras(self.camera, extrins, intrins)
        first = [cam_of.index(c) for c in range(len(homos))]      # a pose of every distinct camera
        rows = self.camera.depth_rows(self.extrins_to_ref(extrins[first]), intrins[first], normalise)
        both = torch.cat([homos.to(torch.float32).reshape(-1), rows.reshape(-1)])      # homographies and rows of every camera: one pinned copy
        if dev.type == "cuda":
            both = both.pin_memory().to(dev, non_blocking=True)
        homos, rows = both[:homos.numel()].view(homos.shape), both[homos.numel():].view(rows.shape)

        def sink(c0, c1):
            part = tuple(b[c0:c1] for b in out)
            return dict(frames8=part[0], depth16=part[1], bg=bg) if display else dict(out=part)

        if fractional:
            chunk = max(1, min(int(max_batch), n))
            segs = [("times", c0, min(n, c0 + chunk)) for c0 in range(0, n, chunk)]
        else:
            segs = path_segments(cam_of, tl, max_batch)
        for kind, c0, c1 in segs:
            if kind == "run":
                if not (0 <= tl[c0] and tl[c1 - 1] < self.frm_num):
                    raise IndexError(f"frame index {tl[c0]} .. {tl[c1 - 1]} outside the clip of {self.frm_num} frames")
                self._rgbd(homos[cam_of[c0]], rows[cam_of[c0]], H, W, run=(tl[c0], c1 - c0), **sink(c0, c1))
            else:
                lo, hi = min(cam_of[c0:c1]), max(cam_of[c0:c1]) + 1      # the chunk's cameras: a slice of the path's
                sel = ([c - lo for c in cam_of[c0:c1]], tl[c0:c1])
                self._rgbd(homos[lo:hi], rows[lo:hi], H, W, **{"times" if kind == "times" else "path": sel}, **sink(c0, c1))
        return tuple(out)

    def display_bg(self):
        """bg_color parsed for the display frames: 3 floats, or None; "random" -- one draw per call, a float composite -- is refused."""
        if self.bg_color == "random":
            raise RuntimeError('render_display: bg_color "random" is one draw per call; the display frames carry a fixed colour (use render)')
        return [float(v) for v in self.bg_color.split('#')] if len(self.bg_color) > 0 else None

    @torch.no_grad()
    def render_display(self, H, W, extrins, intrins, ts, channels=3, out=None, max_batch=64, fractional=False):
        """Poses in, the frames a viewer shows out: N poses (extrins [N,4,4] world-to-camera, intrins [N,3,3]), output frame i showing frame
        ts[i] of the clip -> uint8 [N,H,W,channels] on the device (`out`: written in place), display_frames of render / render_path byte
        for byte, stored by the render launches themselves (`frames8=`): no float frame exists.  Equal poses share a camera (path_cameras);
        chunks of at most `max_batch` frames are launched as render_video.path_segments says -- one run call for a chunk that is one run,
        else one path call.  `fractional`: ts are real LOOP TIMES of any sign and size, as render_path takes them; every chunk is one call
        of the path in loop time."""
        from .render_video import path_segments
        extrins = torch.as_tensor(extrins, dtype=torch.float32).cpu()
        intrins = torch.as_tensor(intrins, dtype=torch.float32).cpu()
        if fractional:
            tl = loop_times(torch.as_tensor(ts).reshape(-1).tolist(), self.frm_num)
        else:
            tl = [int(t) for t in torch.as_tensor(ts).reshape(-1).tolist()]
        n, dev = len(tl), self.device
        if not (len(extrins) == len(intrins) == n):
            raise RuntimeError(f"render_display: one pose and one frame per output frame ({len(extrins)} extrins, {len(intrins)} intrins, {n} frames)")
        if channels not in (3, 4):
            raise ValueError(f"render_display: channels must be 3 (RGB8) or 4 (RGBA8), got {channels}")
        bg = self.display_bg()
        if out is None:
            out = torch.empty((n, H, W, channels), dtype=torch.uint8, device=dev)
        elif out.dtype != torch.uint8 or tuple(out.shape) != (n, H, W, channels) or not out.is_contiguous() or out.device != dev:
            raise RuntimeError(f"render_display: `out` must be contiguous uint8 [{n},{H},{W},{channels}] on the model's device")
        if n == 0:
            return out
        cam_of, homos = path_cameras(self.camera, extrins, intrins)
        if dev.type == "cuda":
            homos = homos.pin_memory().to(dev, non_blocking=True)      # [cameras, D, 3, 3], one copy
        if fractional:
            chunk = max(1, min(int(max_batch), n))
            for c0 in range(0, n, chunk):
                c1 = min(n, c0 + chunk)
                lo, hi = min(cam_of[c0:c1]), max(cam_of[c0:c1]) + 1      # the chunk's cameras, as below
                self._times([c - lo for c in cam_of[c0:c1]], tl[c0:c1], homos[lo:hi], H, W, None, frames8=out[c0:c1], bg=bg)
            return out
        for kind, c0, c1 in path_segments(cam_of, tl, max_batch):
            if kind == "run":
                if not (0 <= tl[c0] and tl[c1 - 1] < self.frm_num):
                    raise IndexError(f"frame index {tl[c0]} .. {tl[c1 - 1]} outside the clip of {self.frm_num} frames")
                self._run(tl[c0], c1 - c0, homos[cam_of[c0]], H, W, None, frames8=out[c0:c1], bg=bg)
            else:
                lo, hi = min(cam_of[c0:c1]), max(cam_of[c0:c1]) + 1      # the chunk's cameras: a slice of the path's (a spiral: exactly its own)
                self._path([c - lo for c in cam_of[c0:c1]], tl[c0:c1], homos[lo:hi], H, W, None, frames8=out[c0:c1], bg=bg)
        return out


class BakedMPV(_Baked):
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

    @property
    def device(self):
        return self.texels.device

    def _run(self, frame0, n, homos, H, W, out, **display):
        from .render import render_frame_run_baked
        return render_frame_run_baked(self.texels, frame0, n, homos, H, W, self.spec, out=out, quad_keep=self.quad_keep, **display)

    def _path(self, frame_cam, frame_t, homos, H, W, out, cull_scratch=None, **display):
        from .render import render_path_baked
        return render_path_baked(self.texels, frame_cam, frame_t, homos, H, W, self.spec, out=out, quad_keep=self.quad_keep, cull_scratch=cull_scratch,
                                 **display)

    def _times(self, frame_cam, frame_time, homos, H, W, out, cull_scratch=None, **display):
        from .render import render_times_baked
        return render_times_baked(self.texels, frame_cam, frame_time, homos, H, W, self.spec, out=out, quad_keep=self.quad_keep,
                                  cull_scratch=cull_scratch, **display)

    def _disparity_run(self, frame0, n, homos, rows, H, W, out):
        from .render import render_frame_run_disparity_baked
        return render_frame_run_disparity_baked(self.texels, frame0, n, homos, rows, H, W, self.spec, quad_keep=self.quad_keep, out=out)

    def _disparity_path(self, frame_cam, frame_t, homos, rows, H, W, out):
        from .render import render_path_disparity_baked
        return render_path_disparity_baked(self.texels, frame_cam, frame_t, homos, rows, H, W, self.spec, quad_keep=self.quad_keep, out=out)

    def _rgbd(self, homos, rows, H, W, **sel_and_sink):
        from .render import render_rgbd_baked
        return render_rgbd_baked(self.texels, homos, rows, H, W, self.spec, quad_keep=self.quad_keep, **sel_and_sink)


class BakedPool(_Baked):
    """bake_pool(module)'s product: the playback model of a tile-culled model without a dense clip.  pool [n_slots * 64, 4] uint8 on the device
    (8 x 8-texel blocks, row-major), layout (packed.PackedLayout: the block table -1 | slot << 1 | dynamic), quad_keep [D,QH,QW] uint8, spec,
    bg_color, camera as in BakedMPV; culled_rgba8: the texel (r | g << 8 | b << 16 | a << 24) a block without storage reads as -- the bake of
    (0, 0, 0, tiles.CULLED_ALPHA) under the model's activations.
    Its render is the dense baked render of `unpack_frames`, bit for bit.  Against bake() of the DENSE model that holds only where the dense
    stack agrees with what the pool stores: static quads with the same texels in every frame (the pool keeps frame 0) and culled texels at
    (0, 0, 0, CULLED_ALPHA).  Other values in culled texels show at ~1e-7 in the float render -- a sample on a tile border can tap the
    neighbouring tile with such a weight -- and not in the uint8 frames (docs/kernels/K9_baked_playback.md, "Culled texels")."""

    def __init__(self, pool, layout, quad_keep, spec, bg_color, camera, culled_rgba8, quad_dyn=None):
        self.pool, self.layout, self.quad_keep, self.spec, self.bg_color, self.camera = pool, layout, quad_keep, spec, bg_color, camera
        self.culled_rgba8 = int(culled_rgba8)
        # quad_dyn [D,QH,QW] uint8 or None: the dynamic quads, where the maker knows them (bake_pool, open_viewer_package, trimmed); the render
        # does not read it.  trim_report: what trimmed() found (None on every other pool)
        self.quad_dyn, self.trim_report = quad_dyn, None

    @property
    def nbytes(self):
        """bytes of the pool (256 per slot) plus the block table."""
        return self.pool.numel() * self.pool.element_size() + self.layout.blocks.numel() * self.layout.blocks.element_size()

    @property
    def frm_num(self):
        return int(self.layout.T)

    @property
    def device(self):
        return self.pool.device

    def _run(self, frame0, n, homos, H, W, out, **display):
        from .render import render_frame_run_baked_pool
        return render_frame_run_baked_pool(self.layout, self.pool, frame0, n, homos, H, W, self.spec, out=out, quad_keep=self.quad_keep,
                                           culled_rgba8=self.culled_rgba8, **display)

    def _path(self, frame_cam, frame_t, homos, H, W, out, cull_scratch=None, **display):
        from .render import render_path_baked_pool
        return render_path_baked_pool(self.layout, self.pool, frame_cam, frame_t, homos, H, W, self.spec, out=out, quad_keep=self.quad_keep,
                                      culled_rgba8=self.culled_rgba8, cull_scratch=cull_scratch, **display)

    def _times(self, frame_cam, frame_time, homos, H, W, out, cull_scratch=None, **display):
        from .render import render_times_baked_pool
        return render_times_baked_pool(self.layout, self.pool, frame_cam, frame_time, homos, H, W, self.spec, out=out, quad_keep=self.quad_keep,
                                       culled_rgba8=self.culled_rgba8, cull_scratch=cull_scratch, **display)

    def _disparity_run(self, frame0, n, homos, rows, H, W, out):
        from .render import render_frame_run_disparity_baked_pool
        return render_frame_run_disparity_baked_pool(self.layout, self.pool, frame0, n, homos, rows, H, W, self.spec, out=out,
                                                     quad_keep=self.quad_keep, culled_rgba8=self.culled_rgba8)

    def _disparity_path(self, frame_cam, frame_t, homos, rows, H, W, out):
        from .render import render_path_disparity_baked_pool
        return render_path_disparity_baked_pool(self.layout, self.pool, frame_cam, frame_t, homos, rows, H, W, self.spec, out=out,
                                                quad_keep=self.quad_keep, culled_rgba8=self.culled_rgba8)

    def _rgbd(self, homos, rows, H, W, **sel_and_sink):
        from .render import render_rgbd_baked_pool
        return render_rgbd_baked_pool(self.layout, self.pool, homos, rows, H, W, self.spec, quad_keep=self.quad_keep, culled_rgba8=self.culled_rgba8,
                                      **sel_and_sink)

    @torch.no_grad()
    def unpack_frames(self, frames):
        """-> (D, len(frames), Hs, Ws, 4) uint8: the frames of the dense baked clip this pool stands for; texels of blocks without storage
        hold culled_rgba8.  Plain torch (tests, export): the render does not go through it."""
        frames = [int(t) for t in frames]
        lay = self.layout
        if frames and (min(frames) < 0 or max(frames) >= lay.T):
            raise IndexError(f"frame index out of range [0, {lay.T})")
        culled = [(self.culled_rgba8 >> (8 * k)) & 0xff for k in range(4)]
        return torch.stack([lay.unpack_plane(self.pool, d, frames, culled=culled) for d in range(lay.D)], 0)

    @torch.no_grad()
    def trimmed(self):
        """-> a new BakedPool without what a player provably cannot show (docs/kernels/K9_baked_playback.md "Trimming the pool"): stored blocks
        none of whose texels shows are dropped from the table, dynamic blocks none of whose texels moves keep frame 0 in one static slot, the
        slots are renumbered densely in table order, and quads whose readable texels all have alpha byte 0 in every frame leave `quad_keep`.
        Every frame the result renders has the bits of this pool's frame -- for every selection, sink and tile layout.  The result has a
        table of its own (a PackedLayout copy), `quad_dyn` (uint8 [D,QH,QW]: kept quads some readable texel of which moves) and `trim_report`;
        this pool and its tensors are not touched.  A pool on the host is refused: the classification and the move are HIP kernels."""
        if not self.pool.is_cuda:
            raise RuntimeError("BakedPool.trimmed: the pool is on the host; the trim runs on the device where the baked model lives and renders")
        lay = self.layout
        flags, slots, tclass = trim_classify(lay, self.pool, self.culled_rgba8)
        size = slots.flatten().long()
        start = torch.cumsum(size, 0) - size
        table = torch.where(size > 0, start * 2 + (size > 1).long(), torch.full_like(start, -1)).to(torch.int32).reshape(lay.blocks.shape).contiguous()
        new = copy.copy(lay)      # D, T, Hs, Ws, tile, quad_grid
        new.blocks, new._index_cache = table, {}
        new.n_slots, new.n_static, new.n_dynamic = int(size.sum()), int((size == 1).sum()), int((size > 1).sum())
        if new.n_slots >= 2 ** 30:
            raise RuntimeError("packed pool too large for 31-bit slot indices")
        pool = torch.empty((new.n_slots * 64, 4), dtype=torch.uint8, device=self.pool.device)
        with torch.cuda.device(self.pool.device):
            L.check(L.lib().vl3d_baked_trim_move(lay.D, lay.T, lay.Hs, lay.Ws, L.ptr(lay.blocks), L.ptr(self.pool), lay.n_slots, L.ptr(table),
                                                 L.ptr(pool) if new.n_slots else None, new.n_slots, L.stream_ptr(self.pool.device)), "vl3d_baked_trim_move")
        QH, QW = (int(v) for v in self.quad_keep.shape[1:])
        keep0 = self.quad_keep.to(self.pool.device).bool()
        keep = keep0 & quad_any((flags & 1).bool(), QH, QW, lay.tile)
        dyn = keep & quad_any((tclass & 2).bool(), QH, QW, lay.tile)
        out = BakedPool(pool, new, keep.to(torch.uint8).contiguous(), self.spec, self.bg_color, self.camera, self.culled_rgba8,
                        quad_dyn=dyn.to(torch.uint8).contiguous())
        e = lay.blocks.flatten()
        stored, was_dyn = e >= 0, (e >= 0) & ((e & 1) == 1)
        dyn0 = None if self.quad_dyn is None else (self.quad_dyn.to(self.pool.device).bool() & keep0)
        out.trim_report = {
            "blocks_stored": int(stored.sum()), "blocks_dropped": int((stored & (size == 0)).sum()), "blocks_demoted": int((was_dyn & (size == 1)).sum()),
            "slots_before": int(lay.n_slots), "slots_after": int(new.n_slots), "bytes_before": int(lay.n_slots) * 256, "bytes_after": int(new.n_slots) * 256,
            "quads_before": int(keep0.sum()), "quads_kept": int(keep.sum()), "quads_dropped": int((keep0 & ~keep).sum()),
            "quads_dynamic": int(dyn.sum()), "quads_demoted": None if dyn0 is None else int((dyn0 & keep & ~dyn).sum())}
        return out


def quad_any(texel_map, QH, QW, tile=None):
    """[D,Hs,Ws] bool -> [D,QH,QW] bool: some texel the quad can read is true -- the texels of tiles.quad_to_texel_mask of that quad alone
    (a quad's closed rectangle grown by one texel on the shared-border lattice; its own th x tw tile in the tile-exact layout).  That mask
    is a product of a row set and a column set, so the reduction is two small matrix products of 0 / 1 values."""
    D, Hs, Ws = texel_map.shape
    dev = texel_map.device

    def members(S, n, t):      # [n, S] float: texel index a of the axis is readable from quad index q
        a, q = torch.arange(S, device=dev, dtype=torch.int64), torch.arange(n, device=dev, dtype=torch.int64)[:, None]
        if t:
            return ((a // t)[None] == q).float()
        qi = lambda v: torch.div(v * n, max(S - 1, 1), rounding_mode="floor").clamp(0, n - 1)      # noqa: E731  (tiles.quad_to_texel_mask)
        return ((qi(a - 1)[None] == q) | (qi(a + 1)[None] == q)).float()
    th, tw = tile if (tile is not None and tile[0]) else (0, 0)
    cols = (texel_map.float() @ members(Ws, QW, tw).t()) > 0                  # D,Hs,QW
    return (members(Hs, QH, th) @ cols.float()) > 0                            # D,QH,QW


def trim_classify(layout, pool, culled_rgba8):
    """vl3d_baked_trim_classify on a baked pool -> (flags [D,Hs,Ws] uint8: bit 0 "alpha byte > 0 in some frame", bit 1 "bytes differ from frame
    0 in some frame"; block_slots int32 like layout.blocks: the block's new slot count 0 | 1 | T; texel_class [D,Hs,Ws] uint8: bit 0 show,
    bit 1 moves), all on the pool's device.  The flag map is the entry's scratch."""
    L.check_cuda(pool, layout.blocks)
    if pool.dtype != torch.uint8 or pool.dim() != 2 or pool.shape[1] != 4 or not pool.is_contiguous() or pool.shape[0] != layout.n_slots * 64:
        raise RuntimeError("trim_classify: a contiguous uint8 pool [n_slots * 64, 4] of the layout")
    bl = layout.blocks
    if bl.dtype != torch.int32 or not bl.is_contiguous() or tuple(bl.shape) != (layout.D, -(-layout.Hs // 8), -(-layout.Ws // 8)) or bl.device != pool.device:
        raise RuntimeError("trim_classify: the layout's block table must be contiguous int32 [D, ceil(Hs/8), ceil(Ws/8)] on the pool's device")
    dev = pool.device
    n = int(L.lib().vl3d_baked_trim_scratch_bytes(layout.D, layout.Hs, layout.Ws))
    scratch = torch.empty((n,), dtype=torch.uint8, device=dev)
    slots = torch.empty(bl.shape, dtype=torch.int32, device=dev)
    tclass = torch.empty((layout.D, layout.Hs, layout.Ws), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().vl3d_baked_trim_classify(layout.D, layout.T, layout.Hs, layout.Ws, L.ptr(bl), L.ptr(pool) if layout.n_slots else None,
                                                 layout.n_slots, int(culled_rgba8) & 0xFFFFFFFF, L.ptr(scratch), n, L.ptr(slots), L.ptr(tclass),
                                                 L.stream_ptr(dev)), "vl3d_baked_trim_classify")
    return scratch[:layout.D * layout.Hs * layout.Ws].view(layout.D, layout.Hs, layout.Ws), slots, tclass


def culled_texel_rgba8(rgb_act, alpha_act):
    """the texel a block without storage reads as: the bake (host rule) of (0, 0, 0, tiles.CULLED_ALPHA) under the activations, as the word
    r | g << 8 | b << 16 | a << 24 (BakedPool.culled_rgba8, the `culled_rgba8` of vl3d_render_fwd_baked_pool)."""
    from .tiles import CULLED_ALPHA
    b = bake_texels(torch.tensor([[0.0, 0.0, 0.0, CULLED_ALPHA]], dtype=torch.float32), rgb_act, alpha_act)[0].tolist()
    return b[0] | b[1] << 8 | b[2] << 16 | b[3] << 24


@torch.no_grad()
def bake_pool(module):
    """Tile-culled MPMeshVid -> BakedPool, without a dense uint8 clip and without a float pool of its own.
      a packed model: ONE bake launch over its pool; the layout is the module's (the table cloned);
      a sparsified dense model (either tile layout): the layout pack_() would build from its quad maps, then plane by plane bake the
        plane's (T,Hs,Ws,4) texels and scatter them through the table (static blocks take frame 0, the dense model's convention) -- the bytes
        bake_pool gives after module.pack_().
    A model that is not sparse (nothing to cull: bake() is its playback model), an `atlas_exact` model and a model on the host are refused."""
    from .packed import TS, PackedLayout
    module = getattr(module, "module", module)
    if getattr(module, "atlas_exact", False):
        raise RuntimeError("bake_pool: atlas_exact models sample the reference's atlas cells; the baked render is built for the planar convention")
    if not (getattr(module, "is_sparse", False) and getattr(module, "quad_keep", None) is not None and getattr(module, "quad_dyn", None) is not None):
        raise RuntimeError("bake_pool: the model is not sparse -- no quad maps, nothing to cull: bake() gives its playback model")
    param = module._param() if hasattr(module, "_param") else None
    if param is None or not hasattr(module, "frm_num"):
        raise RuntimeError("bake_pool: an MPMeshVid (its dense (D,T,Hs,Ws,4) stack, or the pool of pack_())")
    if not param.is_cuda:
        raise RuntimeError("bake_pool: the model is on the host; the baked model lives and renders on the device (module.cuda() first)")
    module._flush_deferred_updates()
    dev = param.device
    ra, aa = module.args.rgb_activate, module.args.alpha_activate
    if module.packed is not None:
        lay = copy.copy(module.packed)      # the module's layout with a table of its own: a later lod() / pack_() of the module does not reach it
        lay.blocks, lay._index_cache = module.packed.blocks.clone(), {}
        pool = bake_texels(module.stack_pool.data.view(-1, 4), ra, aa)
    else:
        stack = module.stack.data
        lay = PackedLayout(module.quad_keep.to(dev), module.quad_dyn.to(dev), stack.shape[1], stack.shape[2], stack.shape[3], module.tile_own)
        # texels of a stored block that lie past the plane's last row / column are never written: pack_() leaves them 0.0, which bakes to this
        unset = bake_texels(torch.zeros((1, 4), dtype=torch.float32, device=dev), ra, aa)
        pool = unset.repeat(lay.n_slots * TS * TS, 1)
        for d in range(lay.D):
            lay.pack_plane_(pool, d, bake_texels(stack[d], ra, aa))      # (T,Hs,Ws,4) uint8: one plane at a time, never the clip
    qk = module.quad_keep.to(torch.uint8).contiguous().clone()
    qd = (module.quad_keep.bool() & module.quad_dyn.bool()).to(torch.uint8).contiguous().clone()
    return BakedPool(pool, lay, qk, module.spec, str(module.args.bg_color), _Camera(module), culled_texel_rgba8(ra, aa), quad_dyn=qd)


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


# ---- a viewer package read back --------------------------------------------------------------------------------------------------
class _PackageCamera(_Camera):
    """the camera of an opened viewer package: what _Camera offers (the same `plane_homographies` code object), built from the package's
    files.  The geometry lives in the reference camera's frame (ref_extrin = I); `ref_intrin_mpi` is the pinhole that maps a vertex's
    (x / z, y / z) to LATTICE coordinates of the tile-exact layout -- column c of the vertex grid is lattice c (tw - 1), row r lattice r (th - 1)."""

    def __init__(self, planedepth, step, origin, tile):
        import types
        self.args, self.mpi_d = types.SimpleNamespace(), int(len(planedepth))
        fx, fy = (tile[1] - 1) / step[0], (tile[0] - 1) / step[1]
        self.ref_extrin = torch.eye(4, dtype=torch.float64)
        self.ref_intrin_mpi = torch.tensor([[fx, 0.0, -origin[0] * fx], [0.0, fy, -origin[1] * fy], [0.0, 0.0, 1.0]], dtype=torch.float64).float()
        self.planedepth = torch.as_tensor(planedepth, dtype=torch.float32).clone()


def package_camera(pk):
    """export.read_viewer_package's dict -> (camera, spec) of the opened model: the plane-pixel grid is the tile lattice itself, so the spec is
    RenderSpec.mpv with identity activations (the texels are baked), scale 1, offset 0 and the package's tile."""
    import dataclasses
    from .render import RenderSpec
    spec = dataclasses.replace(RenderSpec.mpv(rgb_act="none", alpha_act="none", scale=(1.0, 1.0), offset=(0.0, 0.0)), tile=tuple(pk["tile"]))
    return _PackageCamera(pk["planedepth"], pk["step"], pk["origin"], pk["tile"]), spec


def atlas_tile_map(tile_src, layout, static_hw, dyn_hw):
    """`tile_src` [D,QH,QW] int32 on the HOST (-1 | k << 1 | dynamic: export.read_viewer_package) checked against the layout and the two atlas
    grids -- every k below (Ah / th) * (Aw / tw) of its atlas -- and uploaded to the layout's device -> what pool_from_atlas_ takes.  An atlas
    of (0, 0) has no tiles."""
    import types
    if layout.tile is None:
        raise RuntimeError("atlas_tile_map: the destination is a tile-exact PackedLayout (tile=(th, tw))")
    th, tw = layout.tile
    ts = torch.as_tensor(tile_src)
    if ts.is_cuda or ts.dtype != torch.int32 or tuple(ts.shape) != (layout.D,) + tuple(layout.quad_grid):
        raise RuntimeError(f"atlas_tile_map: tile_src must be int32 [D,QH,QW] = {(layout.D,) + tuple(layout.quad_grid)} on the host, got {tuple(ts.shape)} {ts.dtype}")
    for mesh, (h, w) in enumerate((static_hw, dyn_hw)):
        if h % th or w % tw or (h == 0) != (w == 0):
            raise RuntimeError(f"atlas_tile_map: an atlas of {h} x {w} texels is no grid of {th} x {tw} tiles")
        k = ts[(ts >= 0) & ((ts & 1) == mesh)] >> 1
        n = (h // th) * (w // tw)
        if k.numel() and int(k.max()) >= n:
            raise RuntimeError(f"atlas_tile_map: tile index {int(k.max())} outside the {'dynamic' if mesh else 'static'} atlas grid of {n} tiles")
    if int(ts.min()) < -1:
        raise RuntimeError("atlas_tile_map: tile_src entries are -1 or k << 1 | dynamic")
    return types.SimpleNamespace(dev=ts.contiguous().to(layout.blocks.device), static_hw=tuple(static_hw), dyn_hw=tuple(dyn_hw))


def pool_from_atlas_(layout, pool, tiles_map, static_atlas, dyn_atlas, frame, culled_rgba8):
    """vl3d_pool_from_atlas_rgba8: one frame of a viewer package's atlases into the baked pool, in place.  layout: the tile-exact PackedLayout
    of the package's quad maps; pool [n_slots * 64, 4] uint8; tiles_map: atlas_tile_map's product; static_atlas [As_h,As_w,4] / dyn_atlas
    [Ad_h,Ad_w,4] uint8 on the device (None for an atlas of (0, 0)), dyn_atlas the dynamic atlas of frame `frame`.  Static blocks are written
    with frame 0 only."""
    L.check_cuda(pool, layout.blocks, tiles_map.dev)
    if pool.dtype != torch.uint8 or pool.dim() != 2 or pool.shape[1] != 4 or not pool.is_contiguous() or pool.shape[0] != layout.n_slots * 64:
        raise RuntimeError("pool_from_atlas_: a contiguous uint8 pool [n_slots * 64, 4] of the layout")
    bl = layout.blocks
    if bl.dtype != torch.int32 or not bl.is_contiguous() or tuple(bl.shape) != (layout.D, -(-layout.Hs // 8), -(-layout.Ws // 8)) or bl.device != pool.device:
        raise RuntimeError("pool_from_atlas_: the layout's block table must be contiguous int32 [D, ceil(Hs/8), ceil(Ws/8)] on the pool's device")
    if not 0 <= int(frame) < layout.T:
        raise IndexError(f"pool_from_atlas_: frame {frame} outside the clip of {layout.T} frames")
    for at, hw in ((static_atlas, tiles_map.static_hw), (dyn_atlas, tiles_map.dyn_hw)):
        if hw == (0, 0):
            if at is not None:
                raise RuntimeError("pool_from_atlas_: an atlas without tiles is passed as None")
            continue
        if at is None or at.dtype != torch.uint8 or tuple(at.shape) != hw + (4,) or not at.is_contiguous() or at.device != pool.device:
            raise RuntimeError(f"pool_from_atlas_: an atlas must be contiguous uint8 [{hw[0]},{hw[1]},4] on the pool's device")
    (th, tw), (QH, QW) = layout.tile, layout.quad_grid
    with torch.cuda.device(pool.device):
        L.check(L.lib().vl3d_pool_from_atlas_rgba8(layout.D, layout.T, layout.Hs, layout.Ws, th, tw, QH, QW, L.ptr(bl), L.ptr(tiles_map.dev),
                                                   L.ptr(static_atlas), *tiles_map.static_hw, L.ptr(dyn_atlas), *tiles_map.dyn_hw, int(frame),
                                                   int(culled_rgba8) & 0xFFFFFFFF, L.ptr(pool), L.stream_ptr(pool.device)),
                "vl3d_pool_from_atlas_rgba8")
    return pool


@torch.no_grad()
def open_viewer_package(dir, device, bg_color="", culled_rgba8=0):
    """A viewer package on disk (export.save_viewer_package: geometry.obj, static.png, dynamic/%04d.png, meta.json) -> BakedPool on `device`,
    from the files alone.  export.read_viewer_package gives the quad maps, the tile of every quad and the camera; the pool is the tile-exact
    PackedLayout of the quad maps.  The static atlas is uploaded once; every dynamic PNG is decoded on a thread pool of at most 16 workers,
    uploaded through pinned memory (two halves of one buffer in turn, so the host copy of frame t + 1 overlaps the upload and scatter of frame
    t) and scattered by one vl3d_pool_from_atlas_rgba8 call per frame: the dense clip never exists, on the host or on the device.  The plane-pixel grid of the returned model is the tile lattice itself: spec = RenderSpec.mpv("none", "none") with
    tile = (th, tw), scale 1, offset 0; the camera's ref_intrin_mpi maps x / z to lattice coordinates (_PackageCamera).  `culled_rgba8`: the
    texel a culled tile reads as (a package does not say; culled_texel_rgba8(...) of the model's activations reproduces bake_pool's bytes)."""
    from concurrent.futures import ThreadPoolExecutor
    from .export import read_png, read_viewer_package
    from .packed import PackedLayout
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("open_viewer_package: the baked model lives and renders on the device (no CPU fallback)")
    pk = read_viewer_package(dir)
    (th, tw), T = pk["tile"], pk["frame_count"]
    keep, dyn = pk["quad_keep"], pk["quad_dyn"]
    D, QH, QW = keep.shape
    lay = PackedLayout(keep.to(dev), dyn.to(dev), T, QH * th, QW * tw, (th, tw))
    tiles_map = atlas_tile_map(pk["tile_src"], lay, *pk["atlas_hw"])
    pool = torch.zeros((lay.n_slots * 64, 4), dtype=torch.uint8, device=dev)

    def load(path, hw, rule):
        img = read_png(path)
        if img.shape != hw + (4,):
            raise RuntimeError(f"open_viewer_package: {path} decodes to {img.shape}, expected {hw + (4,)} (rule: {rule})")
        return img
    s_hw, d_hw = tiles_map.static_hw, tiles_map.dyn_hw
    static = None if s_hw == (0, 0) else torch.from_numpy(load(pk["static_path"], s_hw, "static.png is an RGBA atlas of the size its header states")).to(dev)
    if d_hw == (0, 0):      # no dynamic quads: every block is static, one call
        pool_from_atlas_(lay, pool, tiles_map, static, None, 0, culled_rgba8)
    else:
        rule = "every PNG in dynamic/ is an RGBA atlas of one size"
        pinned = torch.empty((2,) + d_hw + (4,), dtype=torch.uint8).pin_memory()      # two halves in turn
        atlas = torch.empty((2,) + d_hw + (4,), dtype=torch.uint8, device=dev)
        left = [torch.cuda.Event(), torch.cuda.Event()]      # recorded behind the scatter that read a half: the half may be written again
        with torch.cuda.device(dev), ThreadPoolExecutor(max_workers=max(1, min(16, T))) as ex:      # (zlib releases the interpreter lock)
            for t0 in range(0, T, 16):      # 16 decoded atlases on the host at most, never the clip's
                paths = pk["dynamic_paths"][t0:t0 + 16]
                for t, img in enumerate(ex.map(load, paths, [d_hw] * len(paths), [rule] * len(paths)), t0):
                    h = t & 1
                    left[h].synchronize()      # (an event never recorded is complete)
                    pinned[h].copy_(torch.from_numpy(img))
                    atlas[h].copy_(pinned[h], non_blocking=True)
                    pool_from_atlas_(lay, pool, tiles_map, static, atlas[h], t, culled_rgba8)
                    left[h].record()
        torch.cuda.current_stream(dev).synchronize()
    camera, spec = package_camera(pk)
    return BakedPool(pool, lay, keep.to(dev).to(torch.uint8).contiguous(), spec, str(bg_color), camera, culled_rgba8,
                     quad_dyn=(keep & dyn).to(dev).to(torch.uint8).contiguous())
