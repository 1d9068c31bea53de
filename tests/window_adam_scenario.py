"""The run behind tests/test_gpu_window_adam_digest.py and its recipe tests/golden/make_window_adam_digest.py: optim.WindowAdam driven through
its public surface alone -- window_leaf(window, plane_boxes), leaf.grad, step(), flush(), state_dict() -- with gradients from
synth.hash_uniform.  No render is involved, so every kernel on the path (catch-up, step, tile marks, the bound on the deferral) is
deterministic and the sha256 of (p, m, v, last_step) after every step states "the same bits".

14 steps, max_defer = 8 (vl3d_adam_flush_older sweeps at t = 6, 8, 10, 12, 14), a learning rate that changes every step, six windows --
one ending at the ragged plane border, one revisited after six other steps, one with per-plane boxes smaller than the window, one with an
empty box -- and one dense full-plane step at the end (a packed model refuses it: 13 steps there)."""
import hashlib

import numpy as np
import torch

from videoloop3d_amd import synth, tiles
from videoloop3d_amd.optim import WindowAdam
from videoloop3d_amd.packed import PackedLayout

STORAGES = ("dense", "shared", "exact", "packed_shared", "packed_exact")
D, T = 3, 11          # T = 11: the four-frame trips of catch-up / flush and the ten-frame trip of the static sum, each with a tail


def geometry(storage):
    """-> Hs, Ws, quad grid or None, tile or None"""
    if storage == "dense":
        return 36, 52, None, None              # ragged 8-texel bookkeeping tiles in both directions
    if storage.endswith("shared"):
        return 36, 52, (5, 7), None            # shared-border quads
    return 36, 48, (6, 8), (6, 6)              # tile-exact: 6 x 8 tiles of 6 x 6 texels


def quad_maps(QH, QW):
    """some quads culled, every other kept quad dynamic"""
    i = torch.arange(D * QH * QW).reshape(D, QH, QW)
    keep = (i * 7 + i // QW) % 5 != 0
    dyn = keep & ((torch.cumsum(keep.flatten(), 0).reshape(D, QH, QW) % 2) == 1)
    return keep, dyn


def windows(Hs, Ws):
    """name -> ((y0, x0, wh, ww), plane boxes [D,4] = (y0, y1, x0, x1) or None)"""
    def win(y0, y1, x0, x1):
        return (y0, x0, min(y1, Hs) - y0, min(x1, Ws) - x0)
    return {
        "A": (win(0, 16, 0, 24), None),
        "B": (win(8, Hs, 16, Ws), None),                                                         # ends at the ragged plane border
        "C": (win(16, 32, 8, 40), None),
        "D": (win(0, 24, 24, Ws), None),
        "E": (win(8, 24, 0, 16), [(8, 24, 0, 16), (8, 16, 0, 8), (16, 24, 8, 16)]),              # boxes smaller than the window
        "F": (win(24, Hs, 8, 48), [(24, Hs, 8, 48), (24, 24, 8, 8), (24, 32, 16, 40)]),          # an empty box
    }


SCHEDULE = "ABCDEFBACFEDB"      # A comes back at step 8, after six other steps; step 14 is the dense one


def _sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def run(storage, dev):
    """-> {"steps": [{"p", "m", "v", "last_step"} per step], "final": {...}} of sha256 hex digests"""
    Hs, Ws, grid, tile = geometry(storage)
    stack = synth.make_plane_stack(D, T, Hs, Ws, seed=7)
    kw, lay, sel = {}, None, None
    if grid is not None:
        keep, dyn = quad_maps(*grid)
        kw = dict(quad_keep=keep.to(dev), quad_dyn=dyn.to(dev), culled_alpha=tiles.CULLED_ALPHA, tile=tile)
        keep_t = tiles.quad_to_texel_mask(keep, Hs, Ws, tile)
        dyn_t = tiles.quad_to_texel_mask(keep & dyn, Hs, Ws, tile)
        # what is a parameter: every frame of a texel a dynamic quad can read, frame 0 of a texel only static quads can read
        sel = dyn_t[:, None].repeat(1, T, 1, 1)
        sel[:, 0] |= keep_t
        sel = sel.to(dev)
    if storage.startswith("packed"):
        lay, pool = PackedLayout.from_dense(stack, keep, dyn, tile)
        lay.to(dev)
        p = torch.nn.Parameter(pool.to(dev))
        kw["layout"] = lay
    else:
        p = torch.nn.Parameter(stack.to(dev))
    opt = WindowAdam([p], lr=5e-3, betas=(0.9, 0.999), eps=6e-8, max_defer=8, **kw)

    def dense_of(x):
        return x if lay is None else torch.stack([lay.unpack_plane(x, d) for d in range(D)], 0)

    def digests():
        st = opt.state[p]
        out = {}
        for name, x in (("p", p.data), ("m", st["exp_avg"]), ("v", st["exp_avg_sq"])):
            x = dense_of(x)
            out[name] = _sha(x if sel is None else x[sel])
        out["last_step"] = _sha(st["last_step"])
        return out

    wins = windows(Hs, Ws)
    steps = []
    for t, name in enumerate(SCHEDULE, 1):
        window, boxes = wins[name]
        opt.param_groups[0]["lr"] = 5e-3 * (1.0 + 0.25 * (t % 3)) / (1.0 + 0.05 * t)
        leaf = opt.window_leaf(window, None if boxes is None else np.asarray(boxes, dtype=np.int32))
        leaf.grad = (synth.hash_uniform(tuple(leaf.shape), seed=100 + t) - 0.5).to(dev)
        opt.step()
        steps.append(digests())
    if lay is None:      # the dense full-plane step
        opt.param_groups[0]["lr"] = 4e-3
        p.grad = (synth.hash_uniform(tuple(p.shape), seed=99) - 0.5).to(dev)
        opt.step()
        p.grad = None
        steps.append(digests())
    assert opt.t == len(steps)
    opt.flush()
    sd = opt.state_dict()
    (s0,) = sd["state"].values()
    final = {"p": _sha(p.data), "m": _sha(s0["exp_avg"]), "v": _sha(s0["exp_avg_sq"]), "step": float(s0["step"]),
             "last_step": _sha(opt.state[p]["last_step"])}
    return {"steps": steps, "final": final}
