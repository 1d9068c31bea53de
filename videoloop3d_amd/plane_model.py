"""What MPMesh (MPI.py, stage 1) and MPMeshVid (MPV.py, stage 2) share: planes + reference camera, the render spec of a texture size, the
host-side homographies, checkpoint plumbing (camera buffers, quad maps, the reference's checkpoints), the driver hooks that do not depend
on the texture's storage, and the export to the reference's layout.  The texture itself -- `stack` / `stack_mask` / `stack_pool` -- its
optimiser, render(), forward() and objective() stay with the two classes."""
import dataclasses

import numpy as np
import torch
import torch.nn as nn

from .render import RenderSpec
from .utils_mpi import compute_homography, make_depths

# activations the HIP kernels implement (subset of MPI.py:21-31; shipped configs use sigmoid/sigmoid)
ACTIVATES = {'relu': torch.relu, 'sigmoid': torch.sigmoid, 'none': lambda x: x,
             'clamp': lambda x: torch.clamp(x, 0, 1), 'abs': torch.abs}


def get_new_intrin(old_intrin, new_h_start, new_w_start):
    """utils.py:196-200."""
    new_intrin = old_intrin.clone() if isinstance(old_intrin, torch.Tensor) else old_intrin.copy()
    new_intrin[..., 0, 2] -= new_w_start
    new_intrin[..., 1, 2] -= new_h_start
    return new_intrin


class PlaneModel(nn.Module):
    BASE_CONFIG = None       # the shipped configuration the `rgb_mlp_type` refusal cites
    RGB_MLP_TYPES = ("direct",)      # the colour heads the class is built for (MPI.py:99-112, MPV.py:107-121)

    def __init__(self, args, H, W, ref_extrin, ref_intrin, near, far, pixel_center, texel_scale, atlas_exact):
        """MPI.py:36-63 / MPV.py:26-56: plane set-up and the reference camera; the subclass creates the texture."""
        super().__init__()
        self.atlas_exact = bool(atlas_exact)
        self.args = args
        self.mpi_h, self.mpi_w = int(args.mpi_h_scale * H), int(args.mpi_w_scale * W)
        self.mpi_d, self.near, self.far = args.mpi_d, near, far
        self.H, self.W = H, W
        self.rgb_mlp_type = getattr(args, "rgb_mlp_type", "direct")
        if self.rgb_mlp_type not in self.RGB_MLP_TYPES:
            raise RuntimeError(f"rgbmlp_type = {args.rgb_mlp_type} not supported (shipped configs use 'direct', {self.BASE_CONFIG}:28)")
        ref_extrin, ref_intrin = np.asarray(ref_extrin), np.asarray(ref_intrin)
        assert ref_extrin.shape == (4, 4) and ref_intrin.shape == (3, 3)
        self.register_buffer("ref_extrin", torch.tensor(ref_extrin))
        self.register_buffer("ref_intrin", torch.tensor(ref_intrin).float())
        self.register_buffer("planedepth", make_depths(self.mpi_d, near, far).float().flip(0))   # plane 0 = nearest (MPI.py:57, MPV.py:51)
        # intrinsics that map the whole (larger) MPI plane to plane pixels (MPV.py:55-56)
        self.H_start, self.W_start = (self.mpi_h - H) // 2, (self.mpi_w - W) // 2
        self.register_buffer("ref_intrin_mpi", get_new_intrin(self.ref_intrin, -self.H_start, -self.W_start))
        if args.rgb_activate not in ACTIVATES or args.alpha_activate not in ACTIVATES:
            raise RuntimeError(f"activation ({args.rgb_activate}, {args.alpha_activate}) not implemented by the HIP kernels")
        self.rgb_activate, self.alpha_activate = ACTIVATES[args.rgb_activate], ACTIVATES[args.alpha_activate]
        self.texel_scale = tuple(float(v) for v in texel_scale)
        self.spec = dataclasses.replace(RenderSpec.mpv(rgb_act=args.rgb_activate, alpha_act=args.alpha_activate,
                                                       scale=self.texel_scale), pixel_center=float(pixel_center))
        self.optimize_geometry = False
        self.is_sparse, self.has_dyn = False, False
        self.tile_own = None             # (th, tw) when every quad owns its border texels (TILE-EXACT layout of a sparsified REFERENCE checkpoint,
                                         # init_from_mpi); None: neighbouring quads share them
        self._window_opt = None          # the crop-aware optimiser handed out by get_optimizer: training renders go through its window

    # ---- the render spec of a texture size ---------------------------------------------------------------------------------
    def _tile_grid(self, hs, ws):
        """(qh, qw, th, tw) of a tile-exact texture of hs x ws texels per plane, or the class's error."""
        raise NotImplementedError

    def _set_texture_geometry(self, hs, ws):
        """the render spec of a texture of hs x ws texels per plane: the planes keep their extent (MPV.py:75-81: normalised UVs), so the
        plane-pixel -> texel scale follows the texture size; in the tile-exact layout the scale gives the LATTICE coordinate (a quad spans
        tile - 1 of them) and the spec carries the tile size (render.RenderSpec.tile)."""
        if self.tile_own is not None:
            qh, qw, th, tw = self._tile_grid(hs, ws)
            self.tile_own = (th, tw)
            self.spec = dataclasses.replace(self.spec, tile=(th, tw),
                                            scale=(self.texel_scale[0] * (qw * (tw - 1)) / max(self.mpi_w - 1, 1),
                                                   self.texel_scale[1] * (qh * (th - 1)) / max(self.mpi_h - 1, 1)))
            return
        self.spec = dataclasses.replace(self.spec, tile=(0, 0), scale=(self.texel_scale[0] * (ws - 1) / max(self.mpi_w - 1, 1),
                                                                       self.texel_scale[1] * (hs - 1) / max(self.mpi_h - 1, 1)))

    # ---- checkpoints -------------------------------------------------------------------------------------------------------
    def _load_camera(self, state_dict):
        self.ref_extrin.data = state_dict['ref_extrin'].type_as(self.ref_extrin)
        self.ref_intrin.data = state_dict['ref_intrin'].type_as(self.ref_intrin)
        self.planedepth.data = state_dict['planedepth'].type_as(self.planedepth)
        self.ref_intrin_mpi.data = get_new_intrin(self.ref_intrin, -self.H_start, -self.W_start)

    def _set_quad_maps(self, keep, dyn, dev=None):
        """the [D,QH,QW] bool maps of a sparsified model as buffers on `dev`; (None, None) clears them."""
        self.register_buffer("quad_keep", None if keep is None else keep.to(dev).bool())
        self.register_buffer("quad_dyn", None if dyn is None else dyn.to(dev).bool())

    def _from_reference_state(self, state_dict, tile_layout, frm_num):
        """a checkpoint of the REFERENCE (plane meshes + packed texture atlases, MPI.py:207-221 / MPV.py:290-304) as this package's state
        dict: its tiles resampled onto the dense stack, the culled / static / dynamic quad maps recovered from its face lists.  A sparsified
        checkpoint in the "exact" layout arrives tile for tile ("self.tile_own": the tile size `sparsify_faces` wrote)."""
        from . import tiles
        hv, wv = int(self.args.mpi_h_verts), int(self.args.mpi_w_verts)
        layout = tile_layout if tile_layout is not None else getattr(self.args, "tile_layout", "exact")
        if layout not in ("exact", "lattice"):
            raise RuntimeError(f"tile_layout must be 'exact' or 'lattice', got {layout!r}")
        sparse = bool(state_dict.get("self.is_sparse", False))
        tile_ref = tiles.reference_tile_size(state_dict, hv, wv) if sparse else None
        own = layout == "exact" and tile_ref is not None and not self.atlas_exact
        st, keep, dyn = tiles.stack_from_reference_state(state_dict, self.mpi_h, self.mpi_w, hv, wv, frm_num, own_borders=own)
        return {"ref_extrin": state_dict["ref_extrin"], "ref_intrin": state_dict["ref_intrin"], "planedepth": state_dict["planedepth"],
                "stack": st, "quad_keep": keep, "quad_dyn": dyn, "self.is_sparse": sparse, "self.has_dyn": sparse,
                "self.tile_own": tile_ref if own else None}

    # ---- export to the reference's layout (MPI.py:207-261, MPV.py:290-341) -------------------------------------------------------
    def _refuse_sh_export(self, what):
        if self.rgb_mlp_type != "direct":
            raise RuntimeError(f"{what}: the reference's atlas layout of a view-dependent model (rgb_mlp_type = {self.rgb_mlp_type!r}, 13 channels) is "
                               "not written; state_dict() is this package's checkpoint and frontal_stack() the (D,1,Hs,Ws,4) picture save_texture shows")

    def reference_state_dict(self):
        """the state_dict of the REFERENCE's module for these weights: plane meshes + packed (static / dynamic) atlases."""
        self._refuse_sh_export("reference_state_dict")
        self._flush_deferred_updates()
        from .export import reference_state_dict
        return reference_state_dict(self)

    def save_mesh(self, prefix):
        """MPI.py:223-240, MPV.py:306-323."""
        self._refuse_sh_export("save_mesh")
        from .export import save_mesh
        return save_mesh(self, prefix, self.reference_state_dict())

    def save_texture(self, prefix):
        """MPI.py:242-261, MPV.py:325-341 (dynamic frames as PNG files: no imageio / ffmpeg here)."""
        self._refuse_sh_export("save_texture")
        from .export import save_texture
        return save_texture(self, prefix, self.reference_state_dict())

    # ---- driver hooks --------------------------------------------------------------------------------------------------------
    def _flush_deferred_updates(self):
        """the crop-aware Adam defers the zero-gradient updates of texels outside the current crop's window: replay them before
        anything reads the whole stack (checkpoints, lod, evaluation renders)."""
        if self._window_opt is not None:
            self._window_opt.flush()

    def get_lrate(self, step):
        """MPI.py:143-152, MPV.py:216-225."""
        args = self.args
        scaling = 0.1 ** (step / (args.lrate_decay * 1000))
        return [("lr", args.lrate * scaling), ("vertlr", args.lrate * getattr(args, "optimize_verts_gain", 1) * scaling)]

    def update_step(self, step):
        """MPI.py:154-156, MPV.py:227-229; geometry optimisation itself is not on the planar path."""
        if step >= getattr(self.args, "optimize_geo_start", 10000000):
            self.optimize_geometry = True

    # ---- geometry ------------------------------------------------------------------------------------------------------------
    def plane_homographies(self, extrin, intrin):
        """[D,3,3] target pixel -> plane pixel for the view `extrin` (ref -> target, [1,4,4]) / `intrin` [1,3,3]
        (utils_mpi.py:240-273 with src = the reference camera, plane normal (0,0,1), distance = planedepth)."""
        dev = extrin.device
        if dev.type == "cpu" and extrin.dtype == torch.float64 and not extrin.requires_grad and not getattr(self.args, "torch_homographies", False):
            # float64 host poses: the closed form in numpy (utils_mpi.plane_homographies_host) -- the same bits as the torch spelling below at a
            # third of the host time.  (float32 poses, as the reference's drivers hold them, keep the torch operators: their rounding is the
            # reference's own, which the goldens pin.)
            from .utils_mpi import plane_homographies_host
            return plane_homographies_host(self._host_np("ref_intrin_mpi"), self._host_np("planedepth"), extrin[0].numpy(),
                                           torch.as_tensor(intrin)[0].detach().cpu().numpy())
        eye = torch.eye(4, dtype=extrin.dtype, device=dev)[None]
        normal = torch.tensor([0., 0., 1.], dtype=extrin.dtype, device=dev).expand(1, self.mpi_d, 3)
        return compute_homography(eye, self._on(dev, "ref_intrin_mpi")[None].to(extrin.dtype), extrin, intrin.to(dev), normal,
                                  self._on(dev, "planedepth")[None].to(extrin.dtype))[0].float()

    def homography_chain(self, extrin, intrin):
        """plane_homographies' torch spelling in the dtype of `extrin`, not rounded to float32: the differentiable chain pose -> homographies
        whose Jacobian poses.camera_tangents takes in float64.  (A method of its own: plane_homographies is also borrowed as a plain function
        by objects that are no PlaneModel.)"""
        dev = extrin.device
        eye = torch.eye(4, dtype=extrin.dtype, device=dev)[None]
        normal = torch.tensor([0., 0., 1.], dtype=extrin.dtype, device=dev).expand(1, self.mpi_d, 3)
        return compute_homography(eye, self._on(dev, "ref_intrin_mpi")[None].to(extrin.dtype), extrin, intrin.to(dev), normal,
                                  self._on(dev, "planedepth")[None].to(extrin.dtype))[0]

    def _host_np(self, name):
        """numpy mirror of a (small, constant) camera buffer, refreshed when the buffer changes."""
        buf = getattr(self, name)
        cache = self.__dict__.setdefault("_host_np_mirrors", {})
        key = (buf.data_ptr(), buf._version, str(buf.device))
        if cache.get(name, (None,))[0] != key:
            cache[name] = (key, buf.detach().cpu().numpy().copy())
        return cache[name][1]

    def _on(self, dev, name):
        """the (small, constant) camera buffers on the device of the pose tensors: poses that arrive on the HOST (as the DataLoader
        produces them, train_3d.py:190-191, train_3dvid.py:214-216) are turned into homographies there -- the 4 x 4 inverse and the chain
        of small matrix products were ~40 kernel launches per view on the device."""
        buf = getattr(self, name)
        if buf.device == dev:
            return buf
        cache = self.__dict__.setdefault("_host_mirrors", {})
        key = (name, str(dev), buf.data_ptr(), buf._version)
        if cache.get(name, (None,))[0] != key:
            cache[name] = (key, buf.detach().to(dev))
        return cache[name][1]

    # ---- disparity ---------------------------------------------------------------------------------------------------------
    def _disparity_runs(self, ts):
        """the requested frames as runs read in place: [(clip [D,T,Hs,Ws,4] on the device, frame0, n)], in the order of `ts`"""
        raise NotImplementedError

    @torch.no_grad()
    def render_disparity(self, H, W, extrin, intrin, ts=None, normalise=False, by_alpha=False):
        """The depth map beside the picture (MPV.py:385, 463-466; MPI.py:493-494, 563-566: `disp_norm`): per pixel the colour composite's own
        blend weights times the inverse view depth of every plane, from the render kernels (render.render_frame_run_disparity) -- no layer
        tensor, for every layout render() takes in evaluation.  extrin ([4,4] or [B,4,4]) / intrin ([3,3] or [B,3,3]): the ref -> target
        extrinsics and the intrinsics render() receives; `ts`: the frames of a video model (None: all).  normalise: stage 1's normalisation
        between far and near (MPI.py:494); by_alpha: the weights divided by alpha (normalize_blendweight_fordepth, MPI.py:564-565).
        -> (disp [N,H,W], alpha [N,H,W]) float32, N = views x frames.  Forward only."""
        from .render import depth_rows, render_frame_run_disparity
        if self.atlas_exact:
            raise RuntimeError("render_disparity: atlas_exact is a parity mode of the reference's atlas sampling; the disparity kernels sample the "
                               "plane stack (build the model without atlas_exact)")
        if self.spec.act_order != "post":
            raise RuntimeError("render_disparity: a model under the bake rule shows its baked texels: bake it (baked.bake / bake_pool) and call the "
                               "playback model's render_disparity")
        self._flush_deferred_updates()
        extrin, intrin = torch.as_tensor(extrin).detach().cpu(), torch.as_tensor(intrin).detach().cpu()
        extrin, intrin = extrin.reshape(-1, 4, 4), intrin.reshape(-1, 3, 3)
        if len(intrin) != len(extrin):
            raise RuntimeError(f"render_disparity: {len(extrin)} extrinsics and {len(intrin)} intrinsics")
        qk = self.quad_keep if (self.is_sparse and getattr(self, "quad_keep", None) is not None) else None
        runs = self._disparity_runs(ts)
        disps, alphas = [], []
        for b in range(len(extrin)):
            homos = self.plane_homographies(extrin[b:b + 1], intrin[b:b + 1])
            rows = depth_rows(extrin[b], intrin[b], self.planedepth, (self.near, self.far) if normalise else None)
            for clip, frame0, n in runs:
                d, a = render_frame_run_disparity(clip, frame0, n, homos.to(clip.device), rows, H, W, self.spec, quad_keep=qk)
                disps.append(d)
                alphas.append(a)
        disp = disps[0] if len(disps) == 1 else torch.cat(disps)
        alpha = alphas[0] if len(alphas) == 1 else torch.cat(alphas)
        if by_alpha:
            disp = disp / alpha.clamp_min(1e-10)
        return disp, alpha

    # ---- cameras ---------------------------------------------------------------------------------------------------------
    def render_cameras(self, H, W, extrins, intrins, ts=None):
        """The picture as a function of the stack AND of the cameras: extrins [B,4,4] (ref -> target) and intrins [B,3,3], float64 tensors
        that may require a gradient (poses.CameraDeltas) -> (rgb [B*T',H,W,3], alpha [B*T',H,W]), T' = len(ts) (None: every frame).
        Per camera: plane_homographies in its torch spelling (the autograd graph from the pose to the homographies, on the poses' device),
        then render.render_planes, whose backward returns d loss / d homos (vl3d_render_bwd_homos) beside the stack gradient.  With `ts`
        the frames are gathered (stack[:, ts]): a refinement renders a few frames of a few views, not a training step's crop.  No
        regularisers, no background colour, no fused optimiser step -- render() / forward() are the training path and stay as they are.
        Refused: atlas_exact, packed models, the tile-exact layout, the view-dependent colour head (rgb_sh)."""
        from .render import render_planes
        who = "render_cameras"
        if self.atlas_exact:
            raise RuntimeError(f"{who}: atlas_exact is a parity mode of the reference's atlas sampling; the camera gradient is built on the plane stack")
        if getattr(self, "packed", None) is not None:
            raise RuntimeError(f"{who}: a packed model has no dense stack to differentiate through (unpack_() it first)")
        if self.tile_own is not None:
            raise RuntimeError(f"{who}: the camera gradient is not built for the tile-exact layout")
        if self.rgb_mlp_type != "direct":
            raise RuntimeError(f"{who}: the camera gradient is not built for the view-dependent colour head (rgb_mlp_type = {self.rgb_mlp_type!r})")
        self._flush_deferred_updates()
        extrins, intrins = torch.as_tensor(extrins), torch.as_tensor(intrins)
        extrins, intrins = extrins.reshape(-1, 4, 4), intrins.reshape(-1, 3, 3).to(extrins.dtype)
        if len(intrins) != len(extrins):
            raise RuntimeError(f"{who}: {len(extrins)} extrinsics and {len(intrins)} intrinsics")
        stack = self.stack if ts is None else self.stack[:, torch.as_tensor(ts, dtype=torch.long, device=self.stack.device)]
        qk = self.quad_keep if (self.is_sparse and getattr(self, "quad_keep", None) is not None) else None
        rgbs, alphas = [], []
        for b in range(len(extrins)):
            homos = self.plane_homographies(extrins[b:b + 1], intrins[b:b + 1])
            rgb, alpha = render_planes(stack, homos.to(stack.device), H, W, self.spec, quad_keep=qk)
            rgbs.append(rgb)
            alphas.append(alpha)
        return (rgbs[0], alphas[0]) if len(rgbs) == 1 else (torch.cat(rgbs), torch.cat(alphas))

    def camera_normal_equations(self, H, W, extrin, intrin, target, ts=None, learn_focal=False, weight=None, window=(0, 0)):
        """The Gauss-Newton system of one view's photometric residual in its camera (render.render_normal_equations): extrin [4,4]
        (ref -> target) and intrin [3,3] of the view, target [T',H,W,3] (T' = len(ts); None: every frame), weight [T',H,W] or None,
        `window` (row0, col0) of the frame the target covers.  The unknowns are a left twist of the extrinsic and, with `learn_focal`, a log
        focal scale (poses.camera_tangents) -> (A [P,P], b [P], cost) float64 on the stack's device, P = 6 or 7.  The stack is read only.
        Refused: what render_cameras refuses."""
        from .poses import camera_tangents
        from .render import render_normal_equations
        who = "camera_normal_equations"
        if self.atlas_exact:
            raise RuntimeError(f"{who}: atlas_exact is a parity mode of the reference's atlas sampling; the normal equations are built on the plane stack")
        if getattr(self, "packed", None) is not None:
            raise RuntimeError(f"{who}: a packed model has no dense stack to differentiate through (unpack_() it first)")
        if self.tile_own is not None:
            raise RuntimeError(f"{who}: the normal equations are not built for the tile-exact layout")
        if self.rgb_mlp_type != "direct":
            raise RuntimeError(f"{who}: the normal equations are not built for the view-dependent colour head (rgb_mlp_type = {self.rgb_mlp_type!r})")
        self._flush_deferred_updates()
        homos, dhomos = camera_tangents(self, extrin, intrin, learn_focal)
        stack = self.stack.detach()
        if ts is not None:
            stack = stack[:, torch.as_tensor(ts, dtype=torch.long, device=stack.device)]
        qk = self.quad_keep if (self.is_sparse and getattr(self, "quad_keep", None) is not None) else None
        dev = stack.device
        return render_normal_equations(stack, homos.to(dev), dhomos.to(dev), torch.as_tensor(target).to(dev), H, W, self.spec, window=window, quad_keep=qk,
                                       weight=None if weight is None else torch.as_tensor(weight).to(dev))

    def camera_register_equations(self, H, W, extrin, intrin, target, ts=None, learn_focal=False, weight=None, window=(0, 0), long_exposure=False,
                                  brightness=None):
        """The Gauss-Newton system of registering one view against a captured clip (render.render_register_equations): camera_normal_equations
        with `long_exposure` (target [H,W,3], the clip's temporal mean, against the mean of the frames `ts`; weight [H,W] or None) and
        `brightness` = (log_gain, bias), two more unknowns after the camera's, evaluated at that point (None: none)
        -> (A [Q,Q], b [Q], cost) float64 on the stack's device, Q = P (+ 2 with `brightness`).  The stack is read only.
        Refused: what camera_normal_equations refuses."""
        from .poses import camera_tangents
        from .render import render_register_equations
        who = "camera_register_equations"
        if self.atlas_exact:
            raise RuntimeError(f"{who}: atlas_exact is a parity mode of the reference's atlas sampling; the normal equations are built on the plane stack")
        if getattr(self, "packed", None) is not None:
            raise RuntimeError(f"{who}: a packed model has no dense stack to differentiate through (unpack_() it first)")
        if self.tile_own is not None:
            raise RuntimeError(f"{who}: the normal equations are not built for the tile-exact layout")
        if self.rgb_mlp_type != "direct":
            raise RuntimeError(f"{who}: the normal equations are not built for the view-dependent colour head (rgb_mlp_type = {self.rgb_mlp_type!r})")
        self._flush_deferred_updates()
        homos, dhomos = camera_tangents(self, extrin, intrin, learn_focal)
        stack = self.stack.detach()
        if ts is not None:
            stack = stack[:, torch.as_tensor(ts, dtype=torch.long, device=stack.device)]
        qk = self.quad_keep if (self.is_sparse and getattr(self, "quad_keep", None) is not None) else None
        dev = stack.device
        return render_register_equations(stack, homos.to(dev), dhomos.to(dev), torch.as_tensor(target).to(dev), H, W, self.spec, window=window,
                                         quad_keep=qk, weight=None if weight is None else torch.as_tensor(weight).to(dev),
                                         long_exposure=long_exposure, brightness=brightness)

    # ---- render --------------------------------------------------------------------------------------------------------------
    def _composite_bg(self, rgb, alpha):
        """MPI.py:550-556, MPV.py:455-461 (as written): the render over args.bg_color ("" = none, "random" = one draw per call, "r#g#b")."""
        if len(self.args.bg_color) == 0:
            return rgb
        if self.args.bg_color == "random":
            bg = torch.rand(3).type_as(rgb)
        else:
            r, g, b = map(float, self.args.bg_color.split('#'))
            bg = torch.tensor([r, g, b]).type_as(rgb)
        return rgb * alpha[..., None] + bg[None, None, None] * (- alpha[..., None] + 1)
