#!/usr/bin/env python3
"""Fine-tune under the bake rule, end to end (`MPMeshVid.playback_rule_`, include/vl3d.h VL3D_ACT_BAKED): does training under the picture the
viewer package shows improve the picture that ships?  The small shape of examples/playback.py (180 x 320, D = 16, T = 12).
  * a TEACHER with alpha contours at +-6: per plane a moving circular blob, logit +6 inside and -6 outside, smooth colours;
  * targets: the teacher's FLOAT frames at 8 cameras of a spiral, 6 to train on and 2 held out;
  * a STUDENT fitted to the targets under "post" (`--fit` Adam iterations, one camera and the whole clip per iteration);
  * two copies of it trained on for the same `--tune` iterations: the CONTROL under "post", the TREATMENT under "baked";
  * all three baked with `bake()`; their display frames (`render_display`) and their float frames at the held-out cameras are scored with
    `evaluations.view_image_metrics` against the targets' 8-bit frames.
Prints one JSON line: float and shipped PSNR / SSIM of student, control and treatment, and the iterations / s of both rules."""
import argparse
import json
import os
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def run(fit=1500, tune=600, lr_fit=0.1, lr_tune=0.02, dev="cuda:0", models=None):
    """`models`: a dict that receives the three trained modules (student, control, treatment) -- profiles/trim_students.py trims their pools"""
    from videoloop3d_amd import evaluations as E
    from videoloop3d_amd import render_video as RV
    from videoloop3d_amd import synth
    from videoloop3d_amd.baked import bake
    from videoloop3d_amd.MPV import MPMeshVid
    dev = torch.device(dev)
    H, W, D, T, hv, wv, N = 180, 320, 16, 12, 18, 32, 8
    args = types.SimpleNamespace(mpv_frm_num=T, mpv_isloop=True, mpi_h_scale=1.1, mpi_w_scale=1.1, mpi_d=D, mpi_h_verts=hv, mpi_w_verts=wv, atlas_grid_h=4,
                                 init_std=0.02, rgb_mlp_type="direct", rgb_activate="sigmoid", alpha_activate="sigmoid", bg_color="", scale_invariant=True,
                                 fp16=False, swd_patch_size=3, swd_patcht_size=3, swd_stride=2, swd_stridet=1, sparsity_loss_weight=0.0,
                                 rgb_smooth_loss_weight=0.0, a_smooth_loss_weight=0.0, density_loss_weight=0.0, d_smooth_loss_weight=0.0,
                                 optimizer="adam", lrate=0.1, lrate_decay=30)
    K = np.array([[0.9 * W, 0, W / 2], [0, 0.9 * W, H / 2], [0, 0, 1]])

    def new_model(stack=None):
        torch.manual_seed(0)
        m = MPMeshVid(args, H, W, np.eye(4), K, 1.0, 100.0, device=dev).to(dev)
        if stack is not None:
            with torch.no_grad():
                m.stack.copy_(stack)
        return m

    teacher = new_model().eval()
    Dn, Tn, Hs, Ws = teacher.stack.shape[:4]
    with torch.no_grad():
        st = synth.make_plane_stack(Dn, Tn, Hs, Ws, seed=5, device=dev, alpha_bias=0.0)
        yy, xx = torch.meshgrid(torch.arange(Hs, device=dev, dtype=torch.float32), torch.arange(Ws, device=dev, dtype=torch.float32), indexing="ij")
        for d in range(Dn):
            for t in range(Tn):      # a blob per plane, circling a little over the loop: every alpha contour is a -6 | +6 edge
                ang = 2 * np.pi * t / Tn
                cy, cx = Hs * (0.25 + 0.5 * ((7 * d + 3) % 11) / 10) + 6 * np.sin(ang), Ws * (0.15 + 0.7 * ((5 * d + 2) % 13) / 12) + 6 * np.cos(ang)
                rad = Hs * (0.12 + 0.02 * (d % 4))
                st[d, t, :, :, 3] = torch.where((yy - cy) ** 2 + (xx - cx) ** 2 <= rad * rad, 6.0, -6.0)
        teacher.stack.copy_(st)
    ext = np.stack([np.eye(4, dtype=np.float32)] * N)      # eight cameras of the spiral of examples/playback.py
    for i in range(N):
        a = 2 * np.pi * i / N
        ext[i, :3, 3] = [0.05 * np.cos(a), 0.03 * np.sin(a), 0.01 * np.sin(2 * a)]
    intr = np.stack([K.astype(np.float32)] * N)
    train_cams, held_out = [0, 1, 3, 4, 6, 7], [2, 5]
    ts = torch.arange(T)

    def float_frames(model, v):
        """[T,H,W,3] float32: the module's render at camera v (its current rule; a gradient when it trains)"""
        rgb, _ = model.render(H, W, torch.tensor(ext[v:v + 1]), torch.tensor(intr[v:v + 1]), ts)
        return rgb

    with torch.no_grad():
        targets = [float_frames(teacher, v).clone() for v in range(N)]
    targets8 = [RV.to8b(t) for t in targets]

    def train(model, iters, lr):
        model.train()
        opt = torch.optim.Adam([model.stack], lr=lr)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for it in range(iters):
            v = train_cams[it % len(train_cams)]
            loss = (float_frames(model, v) - targets[v]).pow(2).mean()
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        return iters / max(time.perf_counter() - t0, 1e-9), float(loss.detach())

    def score(model):
        """held-out cameras: (psnr, ssim) of the float picture ("post") and of the shipped picture (bake(model)'s display frames)"""
        was = model.playback_rule
        model.playback_rule_(False).eval()
        shipped = bake(model)
        out = {"float": [], "shipped": []}
        with torch.no_grad():
            for v in held_out:
                e, k = np.repeat(ext[v:v + 1], T, 0), np.repeat(intr[v:v + 1], T, 0)
                frames = {"float": RV.to8b(float_frames(model, v)), "shipped": shipped.render_display(H, W, e, k, np.arange(T), channels=3)}
                for name, f in frames.items():
                    psnr, ssim, _ = E.view_image_metrics(targets8[v], f.contiguous())
                    out[name].append((psnr, ssim))
        model.playback_rule_(was)
        return {name: {"psnr_dB": float(np.mean([p for p, _ in vals])), "ssim": float(np.mean([s for _, s in vals]))} for name, vals in out.items()}

    out = {"shape": f"{H}x{W}, D={D}, T={T}, planes {(Hs, Ws)}, {len(train_cams)} training cameras, {len(held_out)} held out",
           "iterations": {"fit": fit, "tune": tune, "lr_fit": lr_fit, "lr_tune": lr_tune}}
    student = new_model()
    _, out["fit_loss"] = train(student, fit, lr_fit)
    out["student"] = score(student)
    control, treatment = new_model(student.stack.data), new_model(student.stack.data)
    treatment.playback_rule_(True)
    its_post, out["control_loss"] = train(control, tune, lr_tune)
    its_baked, out["treatment_loss"] = train(treatment, tune, lr_tune)
    out["control"], out["treatment"] = score(control), score(treatment)
    out["iterations_per_s"] = {"post": its_post, "baked": its_baked}
    out["shipped_psnr_gain_of_treatment_over_control_dB"] = out["treatment"]["shipped"]["psnr_dB"] - out["control"]["shipped"]["psnr_dB"]
    if models is not None:
        models.update(student=student, control=control, treatment=treatment)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--fit", type=int, default=1500, help="iterations of the student's fit under 'post'")
    ap.add_argument("--tune", type=int, default=600, help="iterations of control ('post') and treatment ('baked') each")
    ap.add_argument("--lr-fit", type=float, default=0.1)
    ap.add_argument("--lr-tune", type=float, default=0.02)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    print(json.dumps(run(a.fit, a.tune, a.lr_fit, a.lr_tune)))
