"""The float training render stated against the CPU oracle in fp64 (oracle/mpi_oracle.py: render_planes), for
tests/test_render_statement_cpu.py (conditions on the reference alone, planted faults) and tests/test_gpu_render_fp64.py (the kernels against
it).  Plain torch on the CPU; of the product only RenderSpec and synth are imported.  The coordinates, the unsafe pixels and the conditions
are tests/baked_statement.py's, extended to the utils_mpi convention.

The statement.  MO.render_planes in float64 on the fp32 (or half-rounded) stack values, the fp32 homographies and the fp32 descriptor floats,
all widened; the sparsity sums (sum_k a_k, sum_k a_k^2) and the loop-mask label sum_k w_k sigmoid(sample(mask_k)) (detached weights) from the
same layers; the stack (and mask) gradient by torch autograd of  sum(rgb g_rgb) + sum(alpha g_alpha) + sum(asum g_asum) + sum(label g_label).
The same evaluation in float32 is "the oracle in fp32": the reference's own rounding noise, which sets the bound.

Unsafe pixels.  Coverage and quad membership are step functions of the texel coordinate.  On a perspective scene a pixel is unsafe when for
some plane its fp64 coordinate lies within baked_statement.DELTA = 1e-3 texel of a plane edge or quad boundary; the forward is compared on the
safe pixels, and the output gradients are ZERO at the unsafe ones on both sides (`objective`) -- the backward is linear in them, so every texel
is compared and no tap is forgiven.  An exact-coordinate scene has no unsafe pixel: its fp32 and fp64 coordinates are equal bit for bit
(`coords_exact`, asserted), so coverage is decided alike on both sides, samples exactly on an edge included.

Exact-coordinate scenes (`views`).  Planar convention, scale (1, 1), bottom homography row (0, 0, 1), every other entry dyadic: lattice
(integer shifts, offset -0.5: samples on texel centres and on tx == 0 and tx == Ws - 1), lattice+ / lattice- (offset -0.5 +- 2^-10: taps of
weight exactly 2^-10), minify (1 - 2^-5 with shears of 2^-6), magnify (1 + 2^-4).  `quad_scenes`: a shared-border quad map with quads of 16 x 8
texels and a tile-exact layout with tiles of 17 x 9 (16 x 8 lattice units), both under the lattice view.  In the tile-exact layout the LATTICE
coordinate -- which decides coverage and the quad -- is exact, the oracle's atlas coordinate (a division by Ws - 1) is not: no unsafe pixel,
but the margin of the perspective scenes.

The bound.  Per scene and per output B = m max |oracle in fp32 - oracle in fp64| over what is compared, no floor: m = 4 (M_COORD,
baked_statement.FACTOR) where the oracle's fp32 coordinates round, m = 16 (M_EXACT) where they are exact and the noise is value arithmetic
alone -- the oracle's sigmoid is about 1 ulp, the kernels' a multiply, v_exp_f32, an add and v_rcp_f32, and the backward reads the stored fp32
forward outputs through (S - P) rcp(1 - a).  tests/test_render_statement_cpu.py shows the smallest planted fault at 4 B or more with m = 16:
that is the cap on m.  fp16 stacks: the owner-computes gradient is one fp32 sum rounded once to half: B + 2^-11 |g64| + 2^-25 per texel."""
import dataclasses
import math

import numpy as np
import torch

import baked_statement as BS
from oracle import mpi_oracle as MO
from videoloop3d_amd import synth
from videoloop3d_amd.render import RenderSpec

DELTA = BS.DELTA
M_COORD, M_EXACT = BS.FACTOR, 16.0
D, T, H, W = 4, 3, 33, 131
EXACT_VIEWS = ("lattice", "lattice+", "lattice-", "minify", "magnify")
EPS = 2.0 ** -10


# ---- coordinates, unsafe pixels, conditions: baked_statement's, for both conventions -------------------------------------------------------------
def plane_coords(homos, H, W, spec, Hs, Ws, dtype=torch.float64):
    """(tx, ty) [D,H,W]: the coordinate coverage is decided on (lattice coordinate in the tile-exact layout), as the oracle forms it in `dtype`"""
    if spec.coord_mode == "affine" and dtype == torch.float64:
        return BS.plane_coords(homos, H, W, spec)
    o = BS.oracle_spec(spec)
    xs, ys = MO._homography_source_coords(H, W, homos.to(dtype), o.pixel_center)
    if spec.coord_mode == "utils_mpi":
        return MO._texel_coords_utils_mpi(xs, ys, Hs, Ws)
    return xs * o.scale[0] + o.offset[0], ys * o.scale[1] + o.offset[1]


def coords_exact(scene):
    """the oracle's fp32 coordinates equal its fp64 ones bit for bit"""
    a = plane_coords(scene.homos, scene.H, scene.W, scene.spec, scene.Hs, scene.Ws, torch.float32)
    b = plane_coords(scene.homos, scene.H, scene.W, scene.spec, scene.Hs, scene.Ws, torch.float64)
    return all(x.dtype == torch.float32 and torch.equal(x.double(), y) for x, y in zip(a, b))


def _steps(spec):
    """where the picture is a step function of the coordinate: the hard cut, or the zeros border under sample-then-activate"""
    return spec.border == "hardcut" or spec.act_order == "post"


def unsafe_mask(scene):
    """[H,W] bool.  Exact-coordinate scenes: none.  utils_mpi convention (zeros border, activate-then-sample): the picture is continuous, none."""
    if scene.exact_coverage or not _steps(scene.spec):
        return torch.zeros((scene.H, scene.W), dtype=torch.bool)
    assert scene.spec.coord_mode == "affine" and scene.spec.border == "hardcut"
    return BS.unsafe_mask(scene.homos, scene.H, scene.W, scene.spec, scene.Hs, scene.Ws, scene.keep)


def conditions(scene):
    """baked_statement.conditions (covered share, the four edges, quad borders, tile seams); `unsafe` is this module's"""
    if scene.spec.coord_mode == "affine":
        c = BS.conditions(scene.homos, scene.H, scene.W, scene.spec, scene.Hs, scene.Ws, scene.keep)
    else:
        tx, ty = plane_coords(scene.homos, scene.H, scene.W, scene.spec, scene.Hs, scene.Ws)
        cov = (tx > -1) & (tx < scene.Ws) & (ty > -1) & (ty < scene.Hs)
        c = dict(covered=float(cov.any(0).double().mean()), edge_left=bool((cov & (tx < 1)).any()), edge_right=bool((cov & (tx > scene.Ws - 2)).any()),
                 edge_top=bool((cov & (ty < 1)).any()), edge_bottom=bool((cov & (ty > scene.Hs - 2)).any()))
    c["unsafe"] = float(unsafe_mask(scene).double().mean())
    if scene.exact_coverage and scene.keep is not None:
        # baked_statement.conditions looks for quad borders among ITS safe samples, a DELTA away from every border; here samples sit exactly ON
        # the borders and decide alike in fp32 and fp64: a covered sample on the border of its kept quad to a culled one (quad_border) and
        # to a kept one (tile_seam), to the left or above
        tx, ty = plane_coords(scene.homos, scene.H, scene.W, scene.spec, scene.Hs, scene.Ws)
        cov = BS.coverage(scene.homos, scene.H, scene.W, scene.spec, scene.Hs, scene.Ws, scene.keep)
        qx, qy, _ = BS.quad_of(tx, ty, scene.Hs, scene.Ws, scene.spec, scene.keep)
        k, d = scene.keep.bool(), torch.arange(scene.keep.shape[0])[:, None, None]
        QH, QW = k.shape[1:]
        ux, uy = (scene.spec.tile[1] - 1, scene.spec.tile[0] - 1) if scene.spec.tile[0] else ((scene.Ws - 1) / QW, (scene.Hs - 1) / QH)
        on_l, on_t = cov & (qx > 0) & (tx == qx * ux), cov & (qy > 0) & (ty == qy * uy)
        kl, kt = k[d, qy, (qx - 1).clamp(min=0)], k[d, (qy - 1).clamp(min=0), qx]
        c["quad_border"] = bool((on_l & ~kl).any()) and bool((on_t & ~kt).any())
        c["tile_seam"] = bool((on_l & kl).any()) and bool((on_t & kt).any())
    return c


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Scene:
    """a view of a stack of D planes of Hs x Ws texels: fp32 homographies [D,3,3], the product's RenderSpec (variant 0), the quad map or None.
    exact_coverage: fp32 and fp64 decide coverage alike (no unsafe pixel); m: the bound's margin"""
    name: str
    homos: torch.Tensor
    H: int
    W: int
    Hs: int
    Ws: int
    spec: RenderSpec
    keep: torch.Tensor = None
    exact_coverage: bool = False
    m: float = M_COORD

    def with_spec(self, **kw):
        return dataclasses.replace(self, spec=dataclasses.replace(self.spec, **kw))


def _affine(a, kx, ky, hx, hy):
    return [[a, kx, hx], [ky, a, hy], [0.0, 0.0, 1.0]]


def _ends(d, n_view, n_tex, a, c):
    """the shift that puts the LOW plane edge (even d) or the HIGH one (odd d) c texels inside a view of n_view pixels scaled by a"""
    return -float(c) if d % 2 == 0 else float(math.floor(n_tex - 1 - a * n_view) + c)


def views(Hs, Ws, Hv=H, Wv=W, Dn=D, act=("sigmoid", "sigmoid")):
    """name -> Scene: the five exact-coordinate views and the perspective one of a stack of Hs x Ws texels under an Hv x Wv frame.  Every
    plane has its own shift; even planes leave the frame at the left, odd ones at the right, planes 0, 1 at the top, 2, 3 at the bottom."""
    out = {}
    mk = lambda off: RenderSpec.mpv(rgb_act=act[0], alpha_act=act[1], scale=(1.0, 1.0), offset=off)      # noqa: E731
    for name in EXACT_VIEWS:
        a, k = {"minify": (1 - 2.0 ** -5, 2.0 ** -6), "magnify": (1 + 2.0 ** -4, 0.0)}.get(name, (1.0, 0.0))
        frac = 0.0 if name.startswith("lattice") else 0.125
        hs = []
        for d in range(Dn):
            hx = _ends(d, Wv, Ws, a, 2 + 2 * d) + frac
            hy = _ends(d // 2, Hv, Hs, a, 1 + d) + frac * 2
            hs.append(_affine(a, k if d % 2 else -k, -k if d % 2 else k, hx, hy))
        off = -0.5 + (EPS if name == "lattice+" else -EPS if name == "lattice-" else 0.0)
        out[name] = Scene(name, torch.tensor(hs, dtype=torch.float32), Hv, Wv, Hs, Ws, mk((off, off)), exact_coverage=True, m=M_EXACT)
        assert coords_exact(out[name]), name      # what "exact-coordinate" means: the oracle's fp32 coordinates ARE its fp64 ones
    out["perspective"] = Scene("perspective", perspective_homos(Dn, Hv, Wv), Hv, Wv, Hs, Ws,
                               RenderSpec.mpv(rgb_act=act[0], alpha_act=act[1], scale=(BS.f32(Ws / Wv), BS.f32(Hs / Hv)), offset=(-0.5, 0.25)))
    return out


def perspective_homos(Dn, Hv, Wv):
    """tests/test_gpu_bwd_choice.py's scene: the benchmark camera over Dn planes, times a 2 degree rotation with a 1 % anisotropy and
    perspective terms of 2e-5 / 3e-5 -- through the oracle's compute_homography"""
    ref_e, Kr, tar_e, Kt = synth.make_cameras(Hv, Wv)
    depths = MO.make_depths(Dn, 1.0, 100.0).flip(0)
    h = MO.compute_homography(ref_e[None], Kr[None], tar_e[None], Kt[None], torch.tensor([0., 0., 1.]).expand(1, Dn, 3), depths[None])[0]
    th = math.radians(2.0)
    Rz = torch.tensor([[math.cos(th) * 1.01, -math.sin(th), 1.0], [math.sin(th), math.cos(th) * 0.99, 0.5], [2e-5, -3e-5, 1.0]])
    return (h @ Rz).float()


def utils_mpi_scene(Hs, Ws, Hv=H, Wv=W, Dn=D, act=("sigmoid", "sigmoid")):
    """the perspective scene under the utils_mpi convention (pixel centre 0, p (size - 1) / size, zeros border, activate-then-sample)"""
    return Scene("utils_mpi", perspective_homos(Dn, Hv, Wv), Hv, Wv, Hs, Ws, RenderSpec(rgb_act=act[0], alpha_act=act[1]))


QUAD = dict(shared=dict(Hs=33, Ws=129, QH=4, QW=8, tile=(0, 0)), tile=dict(Hs=36, Ws=136, QH=4, QW=8, tile=(9, 17)))


def quad_keep(Dn=D, QH=4, QW=8):
    keep = synth.hash_uniform((Dn, QH, QW), seed=11) < 0.6
    keep[2, :, :2] = False
    return keep


def quad_scenes(Hv=H, Wv=W, Dn=D):
    """name -> Scene: `shared` (shared-border quad map, quads of 16 x 8 texels) and `tile` (tile-exact, tiles of 17 x 9 texels = 16 x 8 lattice
    units), each under the lattice view and the perspective one.  Spans that are powers of two keep the quad index exact in fp32."""
    out = {}
    for name, g in QUAD.items():
        ext = (g["Hs"], g["Ws"]) if not g["tile"][0] else (g["QH"] * (g["tile"][0] - 1) + 1, g["QW"] * (g["tile"][1] - 1) + 1)
        for vname, v in views(*ext, Hv, Wv, Dn).items():
            if vname in ("lattice", "perspective"):
                exact = vname == "lattice"
                out[f"{name}/{vname}"] = dataclasses.replace(v, name=f"{name}/{vname}", Hs=g["Hs"], Ws=g["Ws"], keep=quad_keep(Dn, g["QH"], g["QW"]),
                                                             spec=dataclasses.replace(v.spec, tile=g["tile"]),
                                                             m=M_EXACT if exact and not g["tile"][0] else M_COORD)
    return out


def make_stack(scene, Tn=T, seed=41, half=False, Dn=D):
    """the stack of a scene: synth.make_plane_stack, float32 (`half`: its values rounded to fp16, still float32)"""
    s = synth.make_plane_stack(Dn, Tn, scene.Hs, scene.Ws, seed=seed)
    return s.half().float() if half else s


# ---- the objective ------------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Objective:
    """output gradients, float32, zero at the unsafe pixels: g_rgb [T,H,W,3], g_alpha [T,H,W], g_asum [T,H,W,2] or None, g_label [T,H,W] or None"""
    g_rgb: torch.Tensor
    g_alpha: torch.Tensor
    g_asum: torch.Tensor = None
    g_label: torch.Tensor = None


def objective(scene, Tn=T, asum=False, label=False, seed=5, unsafe=None):
    """hash-drawn output gradients in [-0.5, 0.5), zero at the unsafe pixels (`unsafe` [H,W] bool: another mask than the scene's own)"""
    safe = (~(unsafe_mask(scene) if unsafe is None else unsafe)).float()
    u = lambda shape, k: (synth.hash_uniform(shape, seed=seed + k) - 0.5) * safe.reshape((1, scene.H, scene.W) + (1,) * (len(shape) - 3))      # noqa: E731
    return Objective(u((Tn, scene.H, scene.W, 3), 0), u((Tn, scene.H, scene.W), 1),
                     u((Tn, scene.H, scene.W, 2), 2) * 0.25 if asum else None, u((Tn, scene.H, scene.W), 3) if label else None)


# ---- a copy of the oracle with faults to plant (dense planar convention) ----------------------------------------------------------------------------
FAULTS = ("drop_taps", "open_edge", "seam_column", "opaque_behind", "sigmoid_1e-5")
SEAM_PLANE, SEAM_COLUMN = 1, 62      # a texel column at the first 62-pixel region seam of the 64-wide backward regions


def _copy_render(stack, homos, Hv, Wv, o, fault=None):
    """MO.render_planes(..., return_layers=True, layer_order='plane') for the dense planar convention, restated so that a fault can be planted;
    without one it gives the oracle's bits (asserted in tests/test_render_statement_cpu.py)"""
    assert o.coord_mode == "affine" and o.border == "hardcut" and o.act_order == "post" and not o.tile[0] and not o.uv_noise_seed
    Dn, Tn, Hs, Ws, _ = stack.shape
    xs, ys = MO._homography_source_coords(Hv, Wv, homos, o.pixel_center)
    tx, ty = xs * o.scale[0] + o.offset[0], ys * o.scale[1] + o.offset[1]
    x0, y0 = torch.floor(tx), torch.floor(ty)
    fx, fy = tx - x0, ty - y0
    x0, y0 = x0.long(), y0.long()
    flat = stack.permute(0, 1, 4, 2, 3).reshape(Dn, Tn * 4, Hs * Ws)
    samp = 0
    for dy, wy in ((0, 1 - fy), (1, fy)):
        for dx, wx in ((0, 1 - fx), (1, fx)):
            xi, yi = x0 + dx, y0 + dy
            ok = (xi >= 0) & (xi < Ws) & (yi >= 0) & (yi < Hs)
            idx = (yi.clamp(0, Hs - 1) * Ws + xi.clamp(0, Ws - 1)).reshape(Dn, 1, -1).expand(Dn, Tn * 4, -1)
            v = torch.gather(flat, 2, idx).reshape(Dn, Tn * 4, Hv, Wv)
            wgt = (wx * wy * ok.to(stack.dtype)).unsqueeze(1)
            term = v * wgt
            if fault == "drop_taps":      # the backward drops taps of weight < 2^-9: the value stays, the gradient goes
                term = torch.where(wgt < 2.0 ** -9, term.detach(), term)
            samp = samp + term
    samp = samp.reshape(Dn, Tn, 4, Hv, Wv)
    sig = (lambda x: torch.sigmoid(x) * (1 + 1e-5)) if fault == "sigmoid_1e-5" else torch.sigmoid
    acts = dict(MO.ACTS, sigmoid=sig)
    samp = torch.cat([acts[o.rgb_act](samp[:, :, :3]), acts[o.alpha_act](samp[:, :, 3:])], dim=2)
    cov = (tx >= 0) & ((tx < Ws - 1) if fault == "open_edge" else (tx <= Ws - 1)) & (ty >= 0) & (ty <= Hs - 1)
    samp = samp * cov[:, None, None].to(samp.dtype)
    layers = samp.permute(1, 3, 4, 0, 2)
    alpha, content = layers[..., 3], layers[..., :3]
    behind = alpha
    if fault == "opaque_behind":      # (S - P) / (1 - a) taken as 0 at a == 1: the planes behind an opaque plane give its alpha no gradient
        behind = torch.where(alpha >= 1, alpha.detach(), alpha)
    trans = torch.cumprod((1 - behind)[..., :-1], dim=-1)
    bw = torch.cat([alpha[..., :1], alpha[..., 1:] * trans], dim=-1)
    return (content * bw.unsqueeze(-1)).sum(dim=-2), bw.sum(-1), bw, layers


# ---- the evaluation -------------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Result:
    rgb: torch.Tensor
    alpha: torch.Tensor
    asum: torch.Tensor = None
    label: torch.Tensor = None
    grad: torch.Tensor = None
    gmask: torch.Tensor = None


def evaluate(scene, stack, obj=None, dtype=torch.float64, mask=None, fault=None, window=(0, 0)):
    """the oracle in `dtype` on `stack` [D,T,Hs,Ws,4] (float32 values) -> Result; with an Objective also the gradients.  mask [D,T,Hs,Ws]: the
    loop-mask logits (label).  window (row0, col0): the H x W window at that corner of a larger frame (integer pixel offsets).  fault: FAULTS"""
    o = BS.oracle_spec(scene.spec)
    s = stack.detach().to(dtype).requires_grad_(obj is not None)
    hom = scene.homos.to(dtype)
    r0, c0 = window
    Hf, Wf = scene.H + r0, scene.W + c0
    if fault in (None, "seam_column"):
        rgb, alpha, bw, layers = MO.render_planes(s, hom, Hf, Wf, o, return_layers=True, quad_keep=scene.keep, layer_order="plane")
    else:
        assert scene.keep is None
        rgb, alpha, bw, layers = _copy_render(s, hom, Hf, Wf, o, fault)
    a = layers[..., 3]
    asum = torch.stack([a.sum(-1), (a * a).sum(-1)], -1)
    m = label = None
    if mask is not None:
        m = mask.detach().to(dtype).requires_grad_(obj is not None)
        ml, _ = MO.sample_layers(torch.stack([m, m, m, m], -1), hom, Hf, Wf, dataclasses.replace(o, rgb_act="sigmoid"), scene.keep)
        label = (bw.detach() * ml[..., 0]).sum(-1)
    crop = lambda x: None if x is None else x[:, r0:, c0:]      # noqa: E731
    res = Result(crop(rgb), crop(alpha), crop(asum), crop(label))
    assert res.rgb.dtype == dtype
    if obj is not None:
        tot = (res.rgb * obj.g_rgb.to(dtype)).sum() + (res.alpha * obj.g_alpha.to(dtype)).sum()
        if obj.g_asum is not None:
            tot = tot + (res.asum * obj.g_asum.to(dtype)).sum()
        if obj.g_label is not None:
            tot = tot + (res.label * obj.g_label.to(dtype)).sum()
        g = torch.autograd.grad(tot, [s] + ([m] if m is not None and obj.g_label is not None else []))
        res.grad = g[0].detach()
        if len(g) > 1:
            res.gmask = g[1].detach()
        if fault == "seam_column":
            res.grad = res.grad.clone()
            res.grad[SEAM_PLANE, :, :, SEAM_COLUMN] = 0
    return Result(*(None if getattr(res, n) is None else getattr(res, n).detach() for n in OUTPUTS))


OUTPUTS = ("rgb", "alpha", "asum", "label", "grad", "gmask")


@dataclasses.dataclass
class Statement:
    """a scene's fp64 statement r64, the oracle's fp32 evaluation r32 of the same, the safe pixels [H,W].  texels [D,Hs,Ws] bool or None: the
    texels whose gradient is compared (a tile-culled model under grad_culled_unwritten: those of kept quads)"""
    scene: Scene
    r64: Result
    r32: Result
    safe: torch.Tensor
    texels: torch.Tensor = None
    half: bool = False

    def _diff(self, name, got):
        """|got - statement| over what is compared of output `name`, and the statement there"""
        ref = getattr(self.r64, name)
        got = got.detach().cpu().double()
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        d = (got - ref).abs()
        if name in ("grad", "gmask"):
            if self.texels is not None:
                sel = self.texels[:, None].expand(ref.shape[:4])
                return d[sel], ref[sel]
            return d.flatten(), ref.flatten()
        sel = self.safe[None].expand(ref.shape[:3])
        return d[sel], ref[sel]

    def noise(self, name):
        d, _ = self._diff(name, getattr(self.r32, name))
        return float(d.max()) if d.numel() else 0.0

    def bound(self, name):
        """B = m x noise: no floor"""
        return self.scene.m * self.noise(name)

    def excess(self, name, got):
        """(max |d|, B, max |d| / allowance): the allowance is B, for a half gradient B + 2^-11 |g64| + 2^-25 per texel"""
        d, ref = self._diff(name, got)
        B = self.bound(name)
        if not d.numel():
            return 0.0, B, 0.0
        assert bool(torch.isfinite(d).all()), (self.scene.name, name, "not finite")
        allow = torch.full_like(d, B)
        if self.half and name == "grad":
            allow = allow + 2.0 ** -11 * ref.abs() + 2.0 ** -25
        ratio = torch.where(allow > 0, d / allow, torch.where(d > 0, torch.full_like(d, math.inf), torch.zeros_like(d)))
        return float(d.max()), B, float(ratio.max())

    def ratios(self, got):
        return {n: self.excess(n, getattr(got, n))[2] for n in OUTPUTS if getattr(got, n) is not None and getattr(self.r64, n) is not None}

    def check(self, tag, got, names=None):
        """print every bound and measured maximum, then hold each compared output to its bound"""
        bad = []
        for n in names or OUTPUTS:
            g = getattr(got, n)
            if g is None:
                continue
            e, B, r = self.excess(n, g)
            print(f"[{self.scene.name} | {tag}] {n}: m {self.scene.m:g} B {B:.3e} measured max {e:.3e} (x{r:.2f} of the allowance), max |statement| "
                  f"{float(getattr(self.r64, n).abs().max()):.3e}; unsafe {100 * float((~self.safe).double().mean()):.3f} %")
            if not r <= 1.0:
                bad.append((n, e, B, r))
        assert not bad, (self.scene.name, tag, bad)


_CACHE = {}


def statement(scene, stack, obj=None, mask=None, window=(0, 0), texels=None, half=False, key=None):
    """Statement of (scene, stack, objective); `key`: cache it under (key) -- a reference is computed once and shared"""
    if key is not None and key in _CACHE:
        return _CACHE[key]
    r64 = evaluate(scene, stack, obj, torch.float64, mask, None, window)
    r32 = evaluate(scene, stack, obj, torch.float32, mask, None, window)
    st = Statement(scene, r64, r32, ~unsafe_mask(scene), texels, half)
    if key is not None:
        _CACHE[key] = st
    return st


# ---- value edges ------------------------------------------------------------------------------------------------------------------------------------------
EDGE_LOGITS = (-104.0, -40.0, -17.0, 0.0, 17.0, 40.0, 104.0)


def edge_logit_stack(scene, Tn=T, seed=43):
    """a normal stack with every 5th value replaced by one of EDGE_LOGITS (hash-drawn)"""
    s = make_stack(scene, Tn, seed)
    pick = (synth.hash_uniform(tuple(s.shape), seed=seed + 1) * len(EDGE_LOGITS)).long().clamp(max=len(EDGE_LOGITS) - 1)
    edge = torch.tensor(EDGE_LOGITS)[pick]
    return torch.where(synth.hash_uniform(tuple(s.shape), seed=seed + 2) < 0.2, edge, s)


def opaque_stack(scene, Tn=T, seed=47):
    """identity activations: colours in [0, 1), alphas in [0.02, 0.9], and blocks of 6 x 6 texels of alpha exactly 1 on planes 1 and 2, so that
    blended alphas are exactly 1 in front of other planes"""
    Dn = scene.homos.shape[0]
    s = synth.hash_uniform((Dn, Tn, scene.Hs, scene.Ws, 4), seed=seed)
    s[..., 3] = 0.02 + 0.88 * s[..., 3]
    for d, y, x in ((1, 8, 20), (1, 20, 70), (2, 12, 40), (2, 5, 100), (1, 14, 58)):
        s[d, :, y:y + 6, x:x + 6, 3] = 1.0
    return s
