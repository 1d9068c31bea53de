"""Stage 1's view-dependent colour head (rgb_mlp_type = 'rgb_sh', direct2sh): what needs no GPU.  The statement (tests/sh_statement.py), the ray
matrix and the channel map against golden G21 (tests/golden/make_golden_r08.py: the reference's own SphericalHarmoic_RGB, get_rays_tensor_batches
and MPMesh.direct2sh); the model's storage, refusals and checkpoints; the driver's direct2sh_epoch hook; the ABI rows."""
import os
import re
import types

import numpy as np
import pytest
import torch

import sh_statement as SH
from videoloop3d_amd import MPI as M
from videoloop3d_amd import train_3d as drv
from videoloop3d_amd.MPI import MPMesh
from videoloop3d_amd.MPV import MPMeshVid, atlas_to_stack, stack_to_atlas
from videoloop3d_amd.render import sh_basis, sh_ray_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 24, 32
K = np.array([[30., 0, 16], [0, 30., 12], [0, 0, 1]])


def _args(**kw):
    a = dict(mpi_h_scale=1.0, mpi_w_scale=1.0, mpi_d=3, rgb_mlp_type="direct", rgb_activate="sigmoid", alpha_activate="sigmoid",
             bg_color="", learn_loop_mask=False, mpi_h_verts=4, mpi_w_verts=5, sparsify_rmfirstlayer=0, mpv_frm_num=3, mpv_isloop=True,
             init_std=0.5, scale_invariant=True, fp16=False, swd_patch_size=3, swd_patcht_size=3, swd_stride=2, swd_stridet=1,
             optimizer="adam", lrate=1e-3, lrate_decay=30, add_uv_noise=False)
    a.update(kw)
    return types.SimpleNamespace(**a)


def _mesh(**kw):
    return MPMesh(_args(**kw), H, W, np.eye(4), K, 1.0, 100.0)


# ---- golden G21 ------------------------------------------------------------------------------------------------------------------
def test_statement_head_matches_the_reference(golden):
    g = golden("g21_sh_head.npz")
    got = SH.head(torch.from_numpy(g["sh_feat"]).double(), torch.from_numpy(g["sh_dirs"]).double())
    assert (got - torch.from_numpy(g["sh_rgba"]).double()).abs().max().item() <= 1e-6


def test_channel_map_is_the_references_permutation(golden):
    """reference channel 4 c + k <-> (stack, stack_sh): the head on the product's storage equals the reference's head on its 13 channels"""
    g = golden("g21_sh_head.npz")
    feat, dirs = torch.from_numpy(g["sh_feat"]).double(), torch.from_numpy(g["sh_dirs"]).double()
    st, sh = M.sh_from_reference(feat)
    assert st.shape == (64, 4) and sh.shape == (64, 3, 4) and (sh[..., 3] == 0).all()
    assert torch.equal(M.sh_to_reference(st, sh), feat)
    b = torch.stack([torch.full_like(dirs[:, 0], SH.C0), -SH.C1 * dirs[:, 1], SH.C1 * dirs[:, 2], -SH.C1 * dirs[:, 0]], -1)
    rgb = st[:, :3] * b[:, :1] + (sh[..., :3] * b[:, 1:, None]).sum(1)
    ours = torch.cat([rgb, st[:, 3:]], -1)
    assert (ours - torch.from_numpy(g["sh_rgba"]).double()).abs().max().item() <= 1e-6
    assert sorted(M.SH_REF_OF_STACK + tuple(c for row in M.SH_REF_OF_SH for c in row)) == list(range(13))


def test_ray_matrix_and_basis_match_the_references_rays(golden):
    g = golden("g21_sh_head.npz")
    h, w = int(g["ray_H"]), int(g["ray_W"])
    Kc = torch.from_numpy(g["ray_intrin"])
    for i in range(2):
        E = torch.from_numpy(g["ray_extrin"][i])
        ref = torch.from_numpy(g["ray_dirs"][i]).double()
        m = sh_ray_matrix(E, Kc)
        assert m.dtype == torch.float32 and m.shape == (3, 3) and m.device.type == "cpu"
        assert (m.double() - SH.ray_matrix(E, Kc)).abs().max().item() <= 1e-6
        assert (SH.ray_dirs(SH.ray_matrix(E, Kc), h, w) - ref).abs().max().item() <= 1e-6
        assert (SH.ray_dirs(m.double(), h, w) - ref).abs().max().item() <= 1e-6
        want = torch.stack([torch.full_like(ref[..., 0], SH.C0), -SH.C1 * ref[..., 1], SH.C1 * ref[..., 2], -SH.C1 * ref[..., 0]], -1)
        assert (sh_basis(m.double(), h, w) - want).abs().max().item() <= 1e-6
        assert (SH.basis(m.double(), h, w) - want).abs().max().item() <= 1e-6
        # a window of the frame: the ray's pixel index is the FRAME's
        assert (sh_basis(m.double(), 2, 3, window=(1, 2)) - want[1:3, 2:5]).abs().max().item() <= 1e-6
    assert sh_ray_matrix(torch.from_numpy(g["ray_extrin"][:1]), Kc).shape == (3, 3)      # [1,4,4] as MPMesh.render slices it


def test_direct2sh_matches_the_references_atlas(golden):
    g = golden("g21_sh_head.npz")
    before, after = torch.from_numpy(g["d2sh_before"]), torch.from_numpy(g["d2sh_after"])
    D, Hm, Wm = 2, 6, 8
    m = MPMesh(_args(mpi_d=D, mpi_h_verts=3, mpi_w_verts=4), Hm, Wm, np.eye(4), K, 1.0, 100.0)
    with torch.no_grad():
        m.stack.copy_(atlas_to_stack(before, D, 1))
    m.direct2sh()
    assert m.rgb_mlp_type == "rgb_sh" and tuple(m.stack_sh.shape) == (D, 1, Hm, Wm, 3, 4)
    assert isinstance(m.stack_sh, torch.nn.Parameter) and m.stack_sh.requires_grad
    assert torch.equal(m.stack.detach(), atlas_to_stack(before, D, 1)) and not m.stack_sh.detach().any()      # MPI.py:279-282
    feat = M.sh_to_reference(m.stack.detach(), m.stack_sh.detach())                      # D,1,Hm,Wm,13
    assert torch.equal(stack_to_atlas(feat, 1), after)
    with pytest.raises(RuntimeError, match="already"):
        m.direct2sh()


def test_direct2sh_keep_picture_divides_the_colour_lanes():
    m = _mesh()
    st = m.stack.detach().clone()
    m.direct2sh(keep_picture=True)
    assert torch.equal(m.stack.detach()[..., 3], st[..., 3])
    assert torch.allclose(m.stack.detach()[..., :3] * SH.C0, st[..., :3], rtol=1e-6, atol=0)
    assert torch.allclose(m.frontal_stack(), st, rtol=1e-6, atol=1e-7)                # d = (0,0,1): C0 * rgb + C1 * 0


def test_constructor_initialises_as_the_reference_writes_it(golden):
    g = golden("g21_sh_head.npz")
    m = _mesh(rgb_mlp_type="rgb_sh")
    assert m.rgb_mlp_type == "rgb_sh"
    assert tuple(m.stack.shape) == (3, 1, H, W, 4) and tuple(m.stack_sh.shape) == (3, 1, H, W, 3, 4)
    assert [n for n, _ in m.named_parameters()] == ["stack", "stack_sh"]
    feat = M.sh_to_reference(m.stack.detach(), m.stack_sh.detach())
    ref = torch.from_numpy(g["init_atlas"])[0]                                           # 13,Ah,Aw
    a0 = float(g["alpha_init_val"])
    assert a0 == M.ALPHA_INIT_VAL
    # MPI.py:106-108 as written: ALPHA_INIT_VAL in channel 0 -- red's first coefficient --, every other feature (the alpha included) uniform
    assert (ref[0] == a0).all() and (feat[..., 0] == a0).all() and (m.stack.detach()[..., 0] == a0).all()
    assert ref[1:].min() >= 0 and ref[1:].max() < 1 and feat[..., 1:].min() >= 0 and feat[..., 1:].max() < 1
    assert feat[..., 12].std() > 0.2 and (m.stack_sh.detach()[..., 3] == 0).all()           # alpha uniform; the reserved lane
    assert abs(float(feat[..., 1:].mean()) - float(ref[1:].mean())) < 0.05


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_mpmeshvid_still_refuses():
    with pytest.raises(RuntimeError, match="rgbmlp_type = rgb_sh not supported"):
        MPMeshVid(_args(rgb_mlp_type="rgb_sh"), H, W, np.eye(4), K, 1.0, 100.0)
    with pytest.raises(RuntimeError, match="not supported"):
        _mesh(rgb_mlp_type="rgba_sh")
    sh = _mesh(rgb_mlp_type="rgb_sh")
    vid = MPMeshVid(_args(), H, W, np.eye(4), K, 1.0, 100.0)
    with pytest.raises(RuntimeError, match=r"frontal_stack\(\)"):
        vid.init_from_mpi(sh.state_dict())
    sd = {k: v for k, v in sh.state_dict().items() if k not in ("stack_sh", "self.rgb_mlp_type")}
    sd["stack"] = sh.frontal_stack()
    vid.init_from_mpi(sd)                                                                # the frontal picture is a direct state
    assert torch.equal(vid.stack.detach()[:, 0], sh.frontal_stack()[:, 0])


def test_frontal_stack():
    m = _mesh(rgb_mlp_type="rgb_sh")
    f = m.frontal_stack()
    assert tuple(f.shape) == (3, 1, H, W, 4)
    want = SH.C0 * m.stack.detach()[..., :3] + SH.C1 * m.stack_sh.detach()[..., 1, :3]
    assert torch.allclose(f[..., :3], want, atol=1e-7) and torch.equal(f[..., 3], m.stack.detach()[..., 3])
    d = _mesh()
    assert torch.equal(d.frontal_stack(), d.stack.detach())


def test_refusals_of_an_sh_model(tmp_path):
    with pytest.raises(RuntimeError, match="atlas_exact"):
        MPMesh(_args(rgb_mlp_type="rgb_sh", atlas_grid_h=1), H, W, np.eye(4), K, 1.0, 100.0, atlas_exact=True)
    ex = MPMesh(_args(atlas_grid_h=1), H, W, np.eye(4), K, 1.0, 100.0, atlas_exact=True)
    with pytest.raises(RuntimeError, match="atlas_exact"):
        ex.direct2sh()
    m = _mesh(rgb_mlp_type="rgb_sh")
    for call in (m.reference_state_dict, lambda: m.save_mesh(str(tmp_path / "m")), lambda: m.save_texture(str(tmp_path / "t"))):
        with pytest.raises(RuntimeError, match="atlas layout"):
            call()
    # add_uv_noise while training (the render's own check comes before any device work)
    m.args.add_uv_noise = True
    m.train()
    E = torch.eye(4, dtype=torch.float64)[None]
    with pytest.raises(RuntimeError, match="add_uv_noise"):
        m.render(8, 8, E, torch.tensor(K)[None])
    m.args.add_uv_noise = False
    # the crop-aware optimiser
    m.args.crop_aware_adam = True
    with pytest.raises(RuntimeError, match="crop_aware_adam"):
        m.get_optimizer()
    m.args.crop_aware_adam = "auto"
    opt = m.get_optimizer()                                                            # CPU: torch's Adam over both parameters
    assert sum(len(gr["params"]) for gr in opt.param_groups) == 2 and m._window_opt is None
    # a reference checkpoint with a 13-channel atlas
    with pytest.raises(RuntimeError, match="13-channel atlas"):
        _mesh().init_from_mpi({"atlas": torch.zeros(1, 13, 4, 4), "ref_extrin": m.ref_extrin, "ref_intrin": m.ref_intrin, "planedepth": m.planedepth})
    # a state whose head and tensors disagree
    sd = m.state_dict()
    del sd["stack_sh"]
    with pytest.raises(RuntimeError, match="lacks stack_sh"):
        _mesh().init_from_mpi(sd)


def test_state_dict_round_trip_switches_a_direct_model():
    m = _mesh(rgb_mlp_type="rgb_sh", learn_loop_mask=True)
    sd = m.state_dict()
    assert sd["self.rgb_mlp_type"] == "rgb_sh" and tuple(sd["stack_sh"].shape) == (3, 1, H, W, 3, 4)
    assert "self.rgb_mlp_type" not in _mesh().state_dict()                              # a direct model's checkpoint is unchanged
    d = _mesh(learn_loop_mask=True)
    assert not hasattr(d, "stack_sh")
    d.init_from_mpi(sd)
    assert d.rgb_mlp_type == "rgb_sh" and isinstance(d.stack_sh, torch.nn.Parameter)
    assert torch.equal(d.stack.detach(), m.stack.detach()) and torch.equal(d.stack_sh.detach(), m.stack_sh.detach())
    assert torch.equal(d.stack_mask.detach(), m.stack_mask.detach())
    assert sorted(n for n, _ in d.named_parameters()) == ["stack", "stack_mask", "stack_sh"]
    sd2 = d.state_dict()
    assert sorted(sd2.keys()) == sorted(sd.keys())
    # ... and back: a direct state into an SH model
    back = _mesh(rgb_mlp_type="rgb_sh")
    back.init_from_mpi(_mesh().state_dict())
    assert back.rgb_mlp_type == "direct" and not hasattr(back, "stack_sh")
    bad = dict(sd, stack_sh=sd["stack_sh"][:, :, :-1])
    with pytest.raises(RuntimeError, match="stack_sh"):
        _mesh().init_from_mpi(bad)


def test_sparsify_and_culling_read_the_alpha_lane_only():
    m = _mesh(rgb_mlp_type="rgb_sh")
    with torch.no_grad():
        m.stack[..., 3] = -8.0
        m.stack[0, :, :12, :16, 3] = 4.0
    sh0 = m.stack_sh.detach().clone()
    m.sparsify_faces(erode_num=0, alpha_thresh=0.05)
    assert m.is_sparse and bool(m.quad_keep[0].any()) and not bool(m.quad_keep[1:].any())
    assert torch.equal(m.stack_sh.detach(), sh0) and m.rgb_mlp_type == "rgb_sh"


# ---- the driver --------------------------------------------------------------------------------------------------------------------
class _FakeMesh:
    def __init__(self, a):
        self.args, self.calls, self.opts = a, [], 0

    def get_optimizer(self):
        self.opts += 1
        self.calls.append(("get_optimizer", self.opts))
        return types.SimpleNamespace(param_groups=[{"lr": None}], tag=self.opts)

    def get_lrate(self, step):
        return [("lr", 0.1)]

    def sparsify_faces(self, erode_num, alpha_thresh):
        self.calls.append(("sparsify_faces",))

    def direct2sh(self):
        self.calls.append(("direct2sh",))

    def state_dict(self):
        return {}


@pytest.mark.parametrize("d2sh,sparsify", [(2, -1), (2, 2), (-1, 1), (None, -1)])
def test_driver_converts_at_direct2sh_epoch_and_only_then(monkeypatch, d2sh, sparsify):
    a = types.SimpleNamespace(N_iters=4, sparsify_epoch=sparsify, density_loss_epoch=0, density_loss_weight=0.0, patch_h_size=16, patch_w_size=16,
                              patch_h_stride=16, patch_w_stride=16, vid2img_mode="first")
    if d2sh is not None:
        a.direct2sh_epoch = d2sh
    vids = [torch.rand(2, 3, 16, 16)]
    rec = []
    monkeypatch.setattr(drv, "run_iter", lambda nerf, opt, item, args, device: (rec.append((len(nerf.calls), opt.tag)), (torch.zeros(()),) * 3 + ({},))[1])
    mesh = _FakeMesh(a)
    drv.train(mesh, a, vids, torch.eye(4)[None, :3], torch.tensor(K, dtype=torch.float32)[None], 16, 16, device="cpu",
              dynmasks=[torch.ones(16, 16)])
    # train_3d.py:282-290: the sparsify check first, then the conversion, each followed by a new optimiser
    want, n = [("get_optimizer", 1)], 1
    for epoch in range(4):
        if epoch == sparsify:
            n += 1
            want += [("sparsify_faces",), ("get_optimizer", n)]
        if d2sh is not None and epoch == d2sh:
            n += 1
            want += [("direct2sh",), ("get_optimizer", n)]
    assert mesh.calls == want
    # one crop per epoch: every iteration ran on the optimiser handed out last, after the epoch's tasks
    for epoch, (ncalls, tag) in enumerate(rec):
        assert tag == 1 + (sparsify >= 0 and epoch >= sparsify) + (d2sh is not None and d2sh >= 0 and epoch >= d2sh)
    assert len(rec) == 4


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def test_abi_rows_present():
    from videoloop3d_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "vl3d.h")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, nargs in (("vl3d_render_sh_fwd", 12), ("vl3d_render_sh_bwd", 16)):
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][0]) == nargs
        decl = re.search(r"\bint " + name + r"\((.*?)\);", hdr, flags=re.S).group(1)
        assert len(decl.split(",")) == nargs
        assert name in integ
    assert "const vl3d_render_desc *desc" in re.search(r"\bint vl3d_render_sh_fwd\((.*?)\);", hdr, flags=re.S).group(1)
    import __graft_entry__ as g
    g.build()
    assert L.lib().vl3d_version() >= 102 and hasattr(L.lib(), "vl3d_render_sh_fwd") and hasattr(L.lib(), "vl3d_render_sh_bwd")
