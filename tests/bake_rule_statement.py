"""The statement of training under the bake rule (include/vl3d.h VL3D_ACT_BAKED), in plain torch on the CPU oracle -- what
tests/test_bake_rule_train_cpu.py and tests/test_gpu_bake_rule_train.py hold the kernels to.

Per texel and channel, with s the stored logit and u8 the byte the bake rule gives for it:

    a = sigmoid(s);  v = a + (u8 / 255 - a).detach();  MO.render_planes(v, ..., planar convention, activations none / none)

The forward value of v is the decoded byte u8 / 255 -- exactly: u8 / 255 <= a <= 2 u8 / 255 for u8 >= 1, so the difference is exact
(Sterbenz) and the sum is the representable number u8 / 255; for u8 = 0 it is a - a.  Its gradient is sigmoid'(s) from the unrounded a: the
rounding is straight-through.  The bytes are PASSED IN: the GPU tests pass baked.bake_texels(stack on the device), the bytes of the kernel
the render shares its bake rule with, so that a texel within an ulp of a byte boundary cannot round one way here and the other way there."""
import torch

from oracle import mpi_oracle as MO


def oracle_spec(scale=(1.0, 1.0), offset=(0.0, 0.0), tile=(0, 0)):
    """the planar MPV convention with identity activations: the blend of the decoded texels, coverage and composite"""
    return MO.RenderSpec(pixel_center=0.5, coord_mode="affine", border="hardcut", act_order="post", rgb_act="none", alpha_act="none",
                         scale=tuple(scale), offset=tuple(offset), tile=tuple(tile))


def decoded_texels(stack, u8):
    """v of the statement: stack [D,T,Hs,Ws,4] logits (fp32 or fp64, may require a gradient), u8 the baked bytes of the same shape"""
    a = torch.sigmoid(stack)
    return a + (u8.to(a.dtype) / 255 - a).detach()


def render(stack, u8, homos, H, W, scale=(1.0, 1.0), offset=(0.0, 0.0), tile=(0, 0), quad_keep=None, return_layers=False):
    """MO.render_planes of the statement -> (rgb, alpha, blend weights[, layers in hit-slot order])"""
    return MO.render_planes(decoded_texels(stack, u8), homos, H, W, oracle_spec(scale, offset, tile), return_layers=return_layers,
                            quad_keep=quad_keep)
