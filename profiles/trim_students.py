#!/usr/bin/env python3
"""What BakedPool.trimmed() finds after TRAINING: the three students of examples/playback_finetune.py (180 x 320, D = 16, T = 12; the student
fitted under "post", the control tuned on under "post", the treatment under the bake rule).  They are dense models, so each gets the quad maps
"every quad kept, every quad dynamic" and is baked with bake_pool: every block of the pool is dynamic, and the trim decides from the trained bytes
alone.  Prints one JSON line per model: the trim report, and how many texels (and alpha bytes) the host and the device bake rule round
differently -- the number behind baking on the device when save_viewer_package is given quad_maps.  One small synthetic scene: indicative.
  python profiles/trim_students.py [--fit 1500 --tune 600] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--fit", type=int, default=1500)
ap.add_argument("--tune", type=int, default=600)
ap.add_argument("--out", default="")
a = ap.parse_args()

import __graft_entry__ as ge  # noqa: E402
ge.build()
import playback_finetune as PF  # noqa: E402
from videoloop3d_amd.baked import bake_pool, bake_texels  # noqa: E402

models, res = {}, {}
res["finetune"] = PF.run(a.fit, a.tune, models=models)
for name, m in models.items():
    m.playback_rule_(False).eval()
    dev = m.stack.device
    ones = torch.ones((m.stack.shape[0], int(m.args.mpi_h_verts) - 1, int(m.args.mpi_w_verts) - 1), dtype=torch.bool)
    m._set_quad_maps(ones, ones.clone(), dev)
    m.is_sparse = m.has_dyn = True
    pool = bake_pool(m)
    torch.cuda.synchronize()
    lean = pool.trimmed()
    torch.cuda.synchronize()
    ra, aa = m.args.rgb_activate, m.args.alpha_activate
    on_dev, on_host = bake_texels(m.stack.data, ra, aa).cpu(), bake_texels(m.stack.data.cpu(), ra, aa)
    diff = on_dev != on_host
    res[name] = {"report": lean.trim_report, "pool_MB": {"before": pool.nbytes / 1e6, "after": lean.nbytes / 1e6},
                 "host_vs_device_bake": {"texels": int(diff[..., 0].numel()), "texels_differing": int(diff.any(-1).sum()),
                                         "alpha_bytes_differing": int(diff[..., 3].sum()),
                                         "alpha_bytes_differing_between_0_and_1": int((diff[..., 3] & (torch.minimum(on_dev[..., 3], on_host[..., 3]) == 0)).sum())}}
    print(json.dumps({name: res[name]}))
if a.out:
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
