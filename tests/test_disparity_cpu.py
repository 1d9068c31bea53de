"""The disparity map off the device: render.depth_rows against the oracle's inverse view depth, the statement of tests/disparity_statement.py
against the stage-1 golden that pins the reference's own `disp_norm`, the conditions that make the scenes of tests/test_gpu_disparity.py a
test (few unsafe pixels; the comparison fails under planted faults), and every refusal of the three C entries (they refuse before anything
touches a device, so the pointers are placeholders nothing reads -- which is why those rows do not run where a device exists; there
tests/test_gpu_disparity.py calls the same rows on real buffers).  No GPU."""
import math

import pytest
import torch

import baked_statement as BS
import disparity_models as DM
import disparity_statement as DS
import refmod as RM
from oracle import mpi_oracle as MO, mpv_oracle
from videoloop3d_amd.render import depth_rows

R4 = RM.R4
no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="placeholder addresses: a refusal that went missing would launch a kernel on them")


# ---- depth_rows --------------------------------------------------------------------------------------------------------------------------
def _camera(seed):
    """a rotated, translated, cropped camera: (ref -> target extrinsic [4,4] float64, crop intrinsics [3,3], plane depths [6], the plane
    camera's intrinsics, h, w)"""
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi: float(torch.rand(1, generator=g)) * (hi - lo) + lo      # noqa: E731
    ax, ay, az = (math.radians(u(-4, 4)) for _ in range(3))
    Rx = torch.tensor([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]], dtype=torch.float64)
    Ry = torch.tensor([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]], dtype=torch.float64)
    Rz = torch.tensor([[math.cos(az), -math.sin(az), 0], [math.sin(az), math.cos(az), 0], [0, 0, 1]], dtype=torch.float64)
    E = torch.eye(4, dtype=torch.float64)
    E[:3, :3] = Rz @ Ry @ Rx
    E[:3, 3] = torch.tensor([u(-0.1, 0.1), u(-0.1, 0.1), u(-0.05, 0.05)], dtype=torch.float64)
    h, w = 23, 31
    K = torch.tensor([[40.0, 0, 30.0 - u(2, 9)], [0, 42.0, 20.0 - u(2, 7)], [0, 0, 1]], dtype=torch.float64)      # (the crop's shifted principal point)
    K_mpi = torch.tensor([[40.0, 0, 33.0], [0, 42.0, 22.0], [0, 0, 1]], dtype=torch.float64)
    return E, K, MO.make_depths(6, 1.0, 100.0).flip(0), K_mpi, h, w


def _oracle_rho(E, K, z, K_mpi, h, w, pc):
    """oracle.mpv_oracle._inv_depth [h,w,D] float32 through the oracle's own homographies"""
    homos = mpv_oracle._homos(K_mpi, E[None], K[None], z)      # (formed in float64, rounded to float32 once)
    return mpv_oracle._inv_depth(homos, h, w, K_mpi.float(), z, E.float(), pc)


@pytest.mark.parametrize("pc", [0.5, 0.0])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_depth_rows_against_the_oracles_inverse_depth(seed, pc):
    """bound 2e-7 max|rho|: the oracle returns float32 (relative rounding 6e-8) from float32 homographies"""
    E, K, z, K_mpi, h, w = _camera(seed)
    want = _oracle_rho(E, K, z, K_mpi, h, w, pc).double()
    rows = depth_rows(E, K, z)
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (6, 3)
    got = DS.rho(rows, h, w, pc)
    err, top = float((got - want).abs().max()), float(want.abs().max())
    print(f"seed {seed} pc {pc}: max |rho| {top:.3f}, max |depth_rows - oracle| {err:.3e}, bound {2e-7 * top:.3e}")
    assert 0.5 < top < 2.0 and err <= 2e-7 * top
    # normalised rows against (rho - 1 / far) / (1 / near - 1 / far)
    near, far = 1.0, 100.0
    got_n = DS.rho(depth_rows(E, K, z, normalise=(near, far)), h, w, pc)
    want_n = (want - 1 / far) / (1 / near - 1 / far)
    assert float((got_n - want_n).abs().max()) <= 2e-7 * max(top, float(want_n.abs().max())) / (1 / near - 1 / far)


def test_depth_rows_of_many_cameras_equal_the_per_camera_rows():
    cams = [_camera(s) for s in (4, 5, 6)]
    z = cams[0][2]
    E, K = torch.stack([c[0] for c in cams]), torch.stack([c[1] for c in cams])
    many = depth_rows(E, K, z)
    assert tuple(many.shape) == (3, 6, 3)
    for i, c in enumerate(cams):
        assert torch.equal(many[i], depth_rows(c[0], c[1], z))
    assert torch.equal(depth_rows(E, K[0], z)[2], depth_rows(E[2], K[0], z))      # one intrinsic matrix for every camera
    assert torch.equal(depth_rows(E, K, z, normalise=(1.0, 100.0))[1], depth_rows(E[1], K[1], z, normalise=(1.0, 100.0)))
    with pytest.raises(RuntimeError, match="depth_rows"):
        depth_rows(E[0], K, z)


# ---- the statement against the reference's own disp_norm (golden G17 a2 / a3) -------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a2", "a3"])
def test_statement_on_the_stage1_golden(tag):
    """G17 pins the reference's `disp_norm` through its edge-weighted d_smooth term (MPI.py:622-637), a2 without and a3 with
    normalize_blendweight_fordepth.  The statement -- normalised rows, compose, / alpha -- in place of the oracle's disparity, on the layers
    the oracle samples from the reference's atlas; tolerance of tests/test_reference_modules_cpu.py: 2e-6 max(1, |golden|)."""
    g15, g = RM.load("g15_sparsify"), RM.load("g17_forward")
    H, W, over, K, ref_extrin, _ = RM.case_A()
    extra_kw = {"a2": dict(l_smooth_loss_weight=0.3, d_smooth_loss_weight=0.1, bg_color="0.2#0.4#0.6"),
                "a3": dict(l_smooth_loss_weight=0.3, d_smooth_loss_weight=0.1, normalize_blendweight_fordepth=True)}[tag]
    args = R4.make_args(learn_loop_mask=True, **{**over, **RM.REG, **extra_kw})
    h, w, tar_e, K_crop, _ = RM.crop_view(g)
    atlas = torch.from_numpy(g15["in_atlas"])
    near, far = 1.0, 100.0
    mpi_h, mpi_w, planedepth, ref_intrin_mpi, extrins = mpv_oracle._geometry(args, args.mpi_d, H, W, ref_extrin, K, near, far, tar_e, atlas.shape[2:4])
    homos = mpv_oracle._homos(ref_intrin_mpi, extrins[0:1], K_crop[0:1], planedepth)
    layers, _ = mpv_oracle._layers(atlas, homos, h, w, args, mpi_h, mpi_w, 0.5, over["atlas_grid_h"], None)      # [1,h,w,D,4]
    rows = depth_rows(extrins[0], K_crop[0], planedepth, normalise=(near, far))
    disp, alpha = DS.compose(layers[..., 3], DS.rho(rows, h, w, 0.5, layers.dtype))
    if tag == "a3":
        disp = disp / alpha.clamp_min(1e-10)
    dg = (disp[:, 1:, :-1] - disp[:, 1:, 1:]).abs() + (disp[:, :-1, 1:] - disp[:, 1:, 1:]).abs()
    c = torch.from_numpy(g[f"{tag}_rgbl"])[:, :3]
    edge = (c[..., 1:, :-1] - c[..., 1:, 1:]).abs().sum(dim=1) + (c[..., :-1, 1:] - c[..., 1:, 1:]).abs().sum(dim=1)
    got = float((dg * (-edge * args.edge_scale + 1).clamp_min(0)).mean())
    want = float(g[f"{tag}_extra_d_smooth"].reshape(-1)[0])
    print(f"{tag}: d_smooth of the statement {got:.8f}, of the reference {want:.8f}")
    assert want > 1e-4 and abs(got - want) <= 2e-6 * max(1.0, abs(want))
    # (the term sees a scaled row: the comparison is not vacuous)
    rows_f = rows.clone()
    rows_f[2] *= 1.5
    disp_f, _ = DS.compose(layers[..., 3], DS.rho(rows_f, h, w, 0.5, layers.dtype))
    assert float((disp_f - DS.compose(layers[..., 3], DS.rho(rows, h, w, 0.5, layers.dtype))[0]).abs().max()) > 1e-3


# ---- the scenes of the GPU tests ------------------------------------------------------------------------------------------------------------
def _float_statements():
    """(scene name, Statement-maker) of every float scene the GPU tests render: fp32 and fp16, sigmoid and clamp (the other activations share their geometry), plus D = 70"""
    out = []
    for dtype in (torch.float32, torch.float16):
        for name, s in DM.float_scenes(dtype).items():
            out.append((f"{name} {dtype}", s))
    for name, s in DM.float_scenes(torch.float32, alpha_act="clamp").items():
        out.append((f"{name} clamp", s))
    out.append(("D = 70", DM.scene_d70()))
    return out


def test_unsafe_share_of_every_scene_is_at_most_one_percent():
    """the cap tests/test_baked_statement_cpu.py holds its scenes to; and the views are non-trivial: planes cover them partly"""
    for name, s in _float_statements():
        for cam in ((DM.CAM70,) if name == "D = 70" else range(3)):
            share = float(BS.unsafe_mask(s.homos[cam], s.H, s.W, s.spec, s.stack.shape[2], s.stack.shape[3], s.keep).double().mean())
            assert share <= 0.01, (name, cam, share)
    for culled in (BS.CULLED, DM.CULLED_VISIBLE):
        for name, s in DM.baked_scenes(culled).items():
            S = s.scene
            for cam in range(3):
                c = S.conditions(cam)
                assert c["unsafe"] <= 0.01 and 0.3 < c["covered"], (name, cam, c)
                assert c["edge_left"] and c["edge_top"] and (c["edge_right"] or c["edge_bottom"]), (name, cam, c)
                if s.kind == "pool":
                    assert c["block_seam_x"] and c["block_seam_y"], (name, cam, c)


def test_unsafe_share_of_the_model_scenes_is_at_most_one_percent():
    """the views tests/test_gpu_disparity.py renders through the models, built here on the host: the tile-exact and the lattice / packed
    MPMeshVid of tests/baked_models.py under model_view, the stage-1 model under its cropped view"""
    import baked_models as BM
    cpu = torch.device("cpu")
    for name, (model, Hm, Wm, K) in (("tile-exact", BM.tile_exact_model(cpu, "")), ("lattice", BM.pool_model(cpu, "", exact=False))):
        ext, Kc = DM.model_view(Hm, Wm, K)
        st = DM.model_statement(name, model, model.stack.detach(), ext, Kc, Hm, Wm, [0])
        assert st.unsafe_share <= 0.01 and 0.3 < float((st.alpha > 0).double().mean()), (name, st.unsafe_share)
    m, _, _, _, _, _, _, ext, Kc, h, w = DM.stage1_model(cpu, "direct")
    st = DM.model_statement("stage 1", m, m.stack.detach(), ext, Kc, h, w, [0])
    assert st.unsafe_share <= 0.01 and 0.3 < float((st.alpha > 0).double().mean()), st.unsafe_share


def test_the_comparison_fails_under_planted_faults():
    """a device output that is the statement's own fp32 evaluation passes; with one plane's row scaled by 1.01, or one coverage bit flipped on
    a safe pixel, it fails -- on a float scene and on a baked one"""
    sel = DM.RUNS["run of 3"]
    sel = BS.run_sel(0, *sel)
    f = DM.float_scenes()["shared keep 0.3"]
    b = DM.baked_scenes()["pool_exact"]
    makers = [("float", lambda **kw: DS.clip_statement(f.name, f.stack, f.homos, kw.pop("rows", f.rows), sel, f.H, f.W, f.spec, f.keep, **kw), f.rows,
               lambda: MO.sample_layers(f.stack[:, 1:2].double(), f.homos[0].double(), f.H, f.W, BS.oracle_spec(f.spec), quad_keep=f.keep)[1]),
              ("baked", lambda **kw: DS.scene_statement(b.scene, kw.pop("rows", b.rows), sel, **kw), b.rows,
               lambda: MO.sample_layers(b.scene.clip[:, 1:2].double(), b.scene.homos[0].double(), b.scene.H, b.scene.W, BS.oracle_spec(b.scene.spec),
                                        quad_keep=b.scene.keep)[1])]
    for kind, make, rows, coverage in makers:
        st = make()
        st.check(f"{kind}: its own fp32 evaluation", st.disp32, st.alpha32)
        assert st.bound[0] > 0 and st.bound[1] > 0
        scaled = rows.clone()
        scaled[0, 1] *= 1.01
        bad = make(rows=scaled)
        with pytest.raises(AssertionError):
            st.check(f"{kind}: plane 1's row scaled by 1.01", bad.disp32, st.alpha32)
        cov = coverage()                                          # [H,W,D] of camera 0
        safe_cov = (cov & st.safe[0][..., None]).nonzero()
        y, x, d = (int(v) for v in safe_cov[len(safe_cov) // 2])
        bad = make(flip=(y, x, d))
        with pytest.raises(AssertionError):
            st.check(f"{kind}: coverage of plane {d} flipped at ({y}, {x})", bad.disp32, bad.alpha32)


# ---- the refusals ------------------------------------------------------------------------------------------------------------------------------
P = 64      # a non-null, 16-byte aligned placeholder
PLACEHOLDERS = dict(stack=P, baked=P, blocks=P, pool=P, homos=P, rows=P, qk=P, cull=P, disp=P, alpha=P, idx=P)


@no_device
@pytest.mark.parametrize("entry, fields, over, status, fragment", [pytest.param(*r[1:], id=f"{r[1][12:]}-{r[0]}") for r in DM.refusal_rows()])
def test_refusals_come_before_the_device(entry, fields, over, status, fragment):
    import __graft_entry__ as g
    g.build()
    rc, msg = DM.call_refusal(entry, DM.refusal_desc(entry, **fields), PLACEHOLDERS, over)
    assert rc == status, (rc, msg)
    assert msg.startswith(entry.encode() + b": ") and fragment in msg, msg


@no_device
@pytest.mark.parametrize("entry", DM.ENTRIES)
def test_a_well_formed_call_gets_as_far_as_the_device(entry):
    """the placeholder call itself is refused by none of the rows: it reaches the launch, which fails without a device"""
    import __graft_entry__ as g
    g.build()
    rc, msg = DM.call_refusal(entry, DM.refusal_desc(entry), PLACEHOLDERS, {})
    assert rc == 2, (rc, msg)                                                   # VL3D_ELAUNCH
