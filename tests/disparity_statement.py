"""The disparity map stated against the CPU oracle in fp64, for tests/test_disparity_cpu.py (conditions on the statement alone) and
tests/test_gpu_disparity.py (the kernels against it).  Plain torch on the CPU; of the product only what tests/baked_statement.py imports
(RenderSpec, synth) is loaded -- no kernel, no wrapper; the affine rows are the caller's, from render.depth_rows, the unit
tests/test_disparity_cpu.py checks against oracle.mpv_oracle._inv_depth.

The statement.  Per output frame
    disp = sum_k bw_k rho_k,   alpha = sum_k bw_k
with bw [H,W,D] the blend weights of MO.overcompose over the layers of MO.sample_layers (warped, activated, coverage-masked: the alpha of a
plane is 0 where the hard cut or the quad map leaves the pixel uncovered), and rho_k(x, y) = row_k . (x + c, y + c, 1) from the fp32 rows
widened.  A float clip enters as its own values widened (an fp16 clip: the half values) under the model's activations; a baked clip as
decoded bytes / 255 under identity activations (baked_statement.Scene: its spec carries them).  The same evaluation with every tensor in
float32 is "the statement in fp32": the oracle's own rounding on the scene, which sets the bound.

Unsafe pixels: baked_statement.unsafe_mask (DELTA = 1e-3 texel from a plane edge or a quad boundary: coverage is a step function there).
The bound: B = 4 max |statement in fp32 - statement in fp64| over the safe pixels, per output (disp, alpha), no floor."""
import dataclasses

import torch

import baked_statement as BS
from oracle import mpi_oracle as MO


def rho(rows, H, W, pixel_center, dtype=torch.float64):
    """[H,W,D]: row_k . (x + c, y + c, 1) of the fp32 rows [D,3] (the centre as float32) in `dtype`"""
    r = rows.to(torch.float32).to(dtype)
    pc = torch.tensor(BS.f32(pixel_center), dtype=dtype)
    y, x = torch.meshgrid(torch.arange(H, dtype=dtype) + pc, torch.arange(W, dtype=dtype) + pc, indexing="ij")
    return r[:, 0] * x[..., None] + r[:, 1] * y[..., None] + r[:, 2]


def compose(a, rho_):
    """alpha x coverage of every plane [...,H,W,D] (plane 0 nearest) and rho [H,W,D] -> (disp [...,H,W], alpha [...,H,W])"""
    bw = MO.overcompose(a, a[..., None])[1]
    return (bw * rho_).sum(-1), bw.sum(-1)


def render(values, homos, rows, H, W, spec, keep=None, dtype=torch.float64, flip=None):
    """one output frame: values [D,Hs,Ws,4] (logits of a float clip, or decoded texels under identity activations), homos [D,3,3], rows [D,3]
    -> (disp [H,W], alpha [H,W]) in `dtype`.  `flip` = (y, x, d): a fault for the tests of the tests -- the coverage of plane d at that pixel
    negated (a covered sample dropped; an uncovered one given alpha 0.5)."""
    layers, cov = MO.sample_layers(values.to(dtype)[:, None], homos.to(dtype), H, W, BS.oracle_spec(spec), quad_keep=keep)
    a = layers[0, ..., 3].clone()                     # [H,W,D]: alpha x coverage
    if flip is not None:
        y, x, d = flip
        a[y, x, d] = 0.0 if bool(cov[y, x, d]) else 0.5
    disp, alpha = compose(a, rho(rows, H, W, spec.pixel_center, dtype))
    assert disp.dtype == dtype and alpha.dtype == dtype
    return disp, alpha


@dataclasses.dataclass
class Statement:
    """the output frames of a selection: the fp64 statement, its fp32 evaluation, the safe pixels [n,H,W]"""
    name: str
    disp: torch.Tensor
    alpha: torch.Tensor
    disp32: torch.Tensor
    alpha32: torch.Tensor
    safe: torch.Tensor

    @property
    def bound(self):
        """(B_disp, B_alpha) = 4 max |fp32 - fp64| over the safe pixels: no floor"""
        if not bool(self.safe.any()):
            return 0.0, 0.0
        return (BS.FACTOR * float((self.disp32.double() - self.disp)[self.safe].abs().max()),
                BS.FACTOR * float((self.alpha32.double() - self.alpha)[self.safe].abs().max()))

    @property
    def unsafe_share(self):
        return float((~self.safe).double().mean())

    def errors(self, disp, alpha):
        disp, alpha = disp.detach().cpu().double(), alpha.detach().cpu().double()
        assert disp.shape == self.disp.shape and alpha.shape == self.alpha.shape, (disp.shape, self.disp.shape)
        if not bool(self.safe.any()):
            return 0.0, 0.0
        return float((disp - self.disp)[self.safe].abs().max()), float((alpha - self.alpha)[self.safe].abs().max())

    def check(self, tag, disp, alpha):
        """print B and the measured maximum, then hold every safe pixel to B -> (e_disp, e_alpha)"""
        (e_d, e_a), (b_d, b_a) = self.errors(disp, alpha), self.bound
        print(f"[{self.name} | {tag}] fp64 statement: B disp {b_d:.3e} alpha {b_a:.3e}; measured max |d disp| {e_d:.3e} |d alpha| {e_a:.3e}; "
              f"max disp {float(self.disp.abs().max()):.3f}; unsafe {100 * self.unsafe_share:.3f} % of {self.safe.numel()} pixels")
        assert e_d <= b_d and e_a <= b_a, (self.name, tag, e_d, b_d, e_a, b_a)
        return e_d, e_a


def statement(name, values_of, homos, rows, sel, H, W, spec, dims, keep=None, **fault):
    """sel: [(cam, t)] -> Statement of those output frames.  values_of(t): the clip's frame t as [D,Hs,Ws,4] values (float64-exact);
    homos [C,D,3,3], rows [C,D,3]; dims = (Hs, Ws) of a plane; `fault`: render's"""
    r64 = [render(values_of(t), homos[c], rows[c], H, W, spec, keep, torch.float64, **fault) for c, t in sel]
    r32 = [render(values_of(t), homos[c], rows[c], H, W, spec, keep, torch.float32, **fault) for c, t in sel]
    unsafe = {c: BS.unsafe_mask(homos[c], H, W, spec, dims[0], dims[1], keep) for c in {c for c, _ in sel}}
    safe = torch.stack([~unsafe[c] for c, _ in sel])
    return Statement(name, torch.stack([d for d, _ in r64]), torch.stack([a for _, a in r64]),
                     torch.stack([d for d, _ in r32]), torch.stack([a for _, a in r32]), safe)


def scene_statement(scene, rows, sel, **fault):
    """the statement of a baked_statement.Scene (a baked clip, or a pool as pool_as_clip restates it): decoded bytes / 255"""
    clip = scene.clip
    return statement(scene.name, lambda t: clip[:, int(t)].double() / 255.0, scene.homos, rows, sel, scene.H, scene.W, scene.spec, scene.dims[2:],
                     scene.keep, **fault)


def clip_statement(name, stack, homos, rows, sel, H, W, spec, keep=None, **fault):
    """the statement of a float clip [D,T,Hs,Ws,4] (float32 or float16: its own values widened) under spec's activations"""
    return statement(name, lambda t: stack[:, int(t)].double(), homos, rows, sel, H, W, spec, tuple(stack.shape[2:4]), keep, **fault)
