"""Training under the bake rule (include/vl3d.h VL3D_ACT_BAKED), the parts that need no device: the spec reaches the descriptor, MPMeshVid
switches its spec and refuses the model kinds bake() refuses, and the statement the GPU tests compare against (tests/bake_rule_statement.py)
says what it is meant to say -- its forward is the render of the decoded bytes, its gradient the activate-first one."""
import dataclasses

import pytest
import torch

import baked_models as BM
import bake_rule_statement as ST
from oracle import mpi_oracle as MO
from videoloop3d_amd import synth


def test_baked_spec_reaches_the_descriptor():
    from videoloop3d_amd import _lib as L
    from videoloop3d_amd.render import RenderSpec, _desc_dims, mask_channel_supported
    assert L.ACT_ORDER == {"pre": 0, "post": 1, "baked": 2}
    spec = dataclasses.replace(RenderSpec.mpv(), act_order="baked")
    d = _desc_dims(4, 2, 40, 72, 37, 70, spec)
    assert d.act_order == 2 and d.coord_mode == L.COORD["affine"] and d.border_mode == L.BORDER["hardcut"]
    assert _desc_dims(4, 2, 40, 72, 37, 70, RenderSpec.mpv()).act_order == 1      # the default is untouched
    assert not mask_channel_supported(torch.zeros(1, 1, 2, 2, 4), spec)


def test_playback_rule_toggles_the_spec_and_refuses_three_model_kinds():
    cpu = torch.device("cpu")
    model, _, _, _ = BM.tile_exact_model(cpu, "")
    keys = sorted(model.state_dict().keys())
    post = model.spec
    assert post.act_order == "post" and not model.playback_rule
    assert model.playback_rule_() is model and model.playback_rule
    assert model.spec == dataclasses.replace(post, act_order="baked")          # nothing else of the spec moves (tile, scale, pixel centre)
    assert sorted(model.state_dict().keys()) == keys                           # the rule is not a parameter
    model._set_texture_geometry(*model.stack.shape[2:4])                       # specs derived from it keep the rule
    assert model.spec.act_order == "baked" and model.spec.tile == post.tile
    with pytest.raises(RuntimeError, match="playback_rule_"):                  # the rule renders the dense stack
        model.pack_()
    model.playback_rule_(False)
    assert model.spec == post
    # refused on: a packed model, an atlas_exact model, activations other than sigmoid / sigmoid -- and the spec stays as it was
    model.pack_()
    with pytest.raises(RuntimeError, match="packed"):
        model.playback_rule_()
    assert model.spec.act_order == "post"
    other, _, _, _ = BM.tile_exact_model(cpu, "")
    other.atlas_exact = True
    with pytest.raises(RuntimeError, match="atlas_exact"):
        other.playback_rule_()
    other.atlas_exact = False
    other.spec = dataclasses.replace(other.spec, rgb_act="none")
    with pytest.raises(RuntimeError, match="sigmoid / sigmoid"):
        other.playback_rule_()
    assert other.spec.act_order == "post"
    other.playback_rule_(False)                                                # switching it off is always possible


def test_train_baked_argument_switches_the_rule_at_construction():
    import numpy as np
    from videoloop3d_amd.MPV import MPMeshVid
    model, Hm, Wm, K = BM.tile_exact_model(torch.device("cpu"), "")
    args = model.args
    assert not MPMeshVid(args, Hm, Wm, np.eye(4), K, 1.0, 100.0).playback_rule
    args.train_baked = True
    assert MPMeshVid(args, Hm, Wm, np.eye(4), K, 1.0, 100.0).spec.act_order == "baked"


def _scene(layout):
    """a fixed scene of tests/baked_models.py on the host: logits, the host rule's bytes, the first camera, the layout's spec and quad map"""
    from videoloop3d_amd.baked import bake_texels
    stack = synth.make_plane_stack(BM.D, 2, BM.HS, BM.WS, seed=7, alpha_bias=-0.5)
    stack[0, :, 8:16, 8:24] = -30.0     # bytes 0 and 255: the two ends of the rule
    stack[1, :, 16:24, 30:50] = 30.0
    keep = synth.hash_uniform((BM.D, BM.QH, BM.QW), seed=11) < 0.5
    keep[2] = False
    import baked_statement as BS
    spec = BM.specs()[layout]
    return stack, bake_texels(stack, "sigmoid", "sigmoid"), BS.cameras(BM.D, BM.H, BM.W)[0], spec, (None if layout == "dense" else keep)


@pytest.mark.parametrize("layout", ["dense", "shared", "exact"])
def test_statement_forward_is_the_render_of_the_decoded_bytes(layout):
    """v = a + (u8 / 255 - a).detach() has the VALUE u8 / 255 exactly (the docstring of tests/bake_rule_statement.py), so the statement's forward
    is MO.render_planes of the baked texels / 255 under identity activations, bit for bit."""
    stack, u8, homos, spec, keep = _scene(layout)
    assert torch.equal(ST.decoded_texels(stack, u8), u8.float() / 255)
    rgb, alpha, _ = ST.render(stack, u8, homos, BM.H, BM.W, spec.scale, spec.offset, spec.tile, keep)
    rgb_b, alpha_b, _ = MO.render_planes(u8.float() / 255, homos, BM.H, BM.W, ST.oracle_spec(spec.scale, spec.offset, spec.tile), quad_keep=keep)
    assert torch.equal(rgb, rgb_b) and torch.equal(alpha, alpha_b)
    assert float(alpha.max()) > 0.3 and int((u8 == 0).sum()) > 0 and int((u8 == 255).sum()) > 0
    # ... and it is NOT the float picture: activation and interpolation do not commute, and the bytes are truncated
    rgb_f, _, _ = MO.render_planes(stack, homos, BM.H, BM.W, dataclasses.replace(ST.oracle_spec(spec.scale, spec.offset, spec.tile), rgb_act="sigmoid",
                                                                               alpha_act="sigmoid"), quad_keep=keep)
    assert float((rgb - rgb_f).abs().max()) > 1e-3


@pytest.mark.parametrize("layout", ["dense", "shared", "exact"])
def test_statement_gradient_is_the_activate_first_one(layout):
    """d loss / d s = sigmoid'(s) * d loss / d v with sigmoid' from the UNROUNDED a: the oracle's gradient with respect to the decoded texels,
    times a (1 - a).  Both sides are fp32 products of the same three numbers in another order: two roundings each, 4 * 2^-24 relative."""
    stack, u8, homos, spec, keep = _scene(layout)
    g_rgb = synth.hash_uniform((2, BM.H, BM.W, 3), seed=5) - 0.5
    g_a = synth.hash_uniform((2, BM.H, BM.W), seed=6) - 0.5
    s = stack.clone().requires_grad_(True)
    rgb, alpha, _ = ST.render(s, u8, homos, BM.H, BM.W, spec.scale, spec.offset, spec.tile, keep)
    (gs,) = torch.autograd.grad([rgb, alpha], s, [g_rgb, g_a])
    v = (u8.float() / 255).requires_grad_(True)
    rgb_v, alpha_v, _ = MO.render_planes(v, homos, BM.H, BM.W, ST.oracle_spec(spec.scale, spec.offset, spec.tile), quad_keep=keep)
    (gv,) = torch.autograd.grad([rgb_v, alpha_v], v, [g_rgb, g_a])
    a = torch.sigmoid(stack)
    want = gv * (a * (1 - a))
    assert float(gs.abs().sum()) > 0
    assert bool(((gs - want).abs() <= 4 * 2.0 ** -24 * want.abs() + 1e-30).all())
