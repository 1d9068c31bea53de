"""The trim rule of a baked pool (docs/kernels/K9_baked_playback.md "Trimming the pool"), stated in plain torch on the host over
baked_statement.pool_as_clip -- for tests/test_baked_trim_cpu.py (the rule against the fp64 oracle) and tests/test_gpu_baked_trim.py (the kernels
and BakedPool.trimmed against the rule).  Of the product only tiles.quad_to_texel_mask is called: the rule names it as the set of texels a quad
can read.  No kernel, no wrapper, no PackedLayout.

The rule, over the in-plane texels of the clip [D,T,Hs,Ws,4] the table stands for (unstored blocks read culled_rgba8):
  A      the largest alpha byte of the T frames;
  show   some texel of the 3 x 3 neighbourhood (clipped to the plane) has A > 0 -- the union of the 2 x 2 bilinear footprints a texel is in;
  moves  show, and the four bytes differ between some frame and frame 0;
  a stored block is DROPPED iff none of its texels shows and the alpha byte of culled_rgba8 is 0;
  a dynamic block that is kept becomes STATIC (frame 0) iff none of its texels moves;
  a kept quad leaves quad_keep iff A == 0 on every texel it can read; it is dynamic iff it stays and one of them moves;
  slots are renumbered in table order, kept blocks copied unchanged."""
import types

import torch

import baked_statement as BS
from videoloop3d_amd import tiles


def edit_scene(st, every_invisible=3, every_frozen=2):
    """a pool storage of baked_models.fp64_scenes() edited so that there is something to trim: every `every_invisible`-th kept quad has alpha byte 0
    on all the texels it can read, in every frame, and every `every_frozen`-th dynamic quad repeats frame 0 on them.  -> (pool, source clip)
    through the storage's own table; the storage is not modified."""
    import baked_models as BM
    D, T, Hs, Ws, _ = st.source.shape
    src = st.source.clone()
    kept = st.keep.flatten().nonzero()[:, 0]
    invisible = torch.zeros(st.keep.numel(), dtype=torch.bool)
    invisible[kept[::every_invisible]] = True
    dyn_q = (st.keep & st.dyn).flatten().nonzero()[:, 0]
    frozen = torch.zeros(st.keep.numel(), dtype=torch.bool)
    frozen[dyn_q[::every_frozen]] = True
    fr = tiles.quad_to_texel_mask(frozen.reshape(st.keep.shape), Hs, Ws, st.tile)
    src = torch.where(fr[:, None, :, :, None], src[:, :1], src)
    inv = tiles.quad_to_texel_mask(invisible.reshape(st.keep.shape), Hs, Ws, st.tile)
    src[..., 3] = torch.where(inv[:, None], torch.zeros_like(src[..., 3]), src[..., 3])
    return BM.scatter_pool(st.lay, src, torch.zeros((1, 4), dtype=torch.uint8)), src


def quad_any(texel_map, quad_shape, tile):
    """[D,Hs,Ws] bool -> [D,QH,QW] bool: true on some texel of tiles.quad_to_texel_mask of that quad alone (one quad position at a time)"""
    D, QH, QW = quad_shape
    Hs, Ws = texel_map.shape[1:]
    out = torch.zeros((D, QH, QW), dtype=torch.bool)
    for qy in range(QH):
        for qx in range(QW):
            one = torch.zeros((D, QH, QW), dtype=torch.bool)
            one[:, qy, qx] = True
            out[:, qy, qx] = (texel_map & tiles.quad_to_texel_mask(one, Hs, Ws, tile)).flatten(1).any(1)
    return out


def texel_maps(clip):
    """clip [D,T,Hs,Ws,4] uint8 -> (A > 0, differs from frame 0, show, moves), each [D,Hs,Ws] bool"""
    vis = clip[..., 3].amax(1) > 0
    dif = (clip != clip[:, :1]).any(-1).any(1)
    show = torch.nn.functional.max_pool2d(vis[:, None].float(), 3, 1, 1)[:, 0] > 0      # (the padding is -inf: out of the plane never counts)
    return vis, dif, show, show & dif


def trim(blocks, pool, T, Hs, Ws, culled_rgba8, quad_keep, tile, own_alpha_only=False):
    """the rule -> namespace: vis, dif, show, moves [D,Hs,Ws] bool; size [D,bh,bw] (0 | 1 | T); dropped, demoted [D,bh,bw] bool; blocks (the new
    table, int32), pool (the new pool), n_slots; keep, dyn [D,QH,QW] bool; clip (the trimmed pool as a clip).
    own_alpha_only: the WRONG variant that drops a block on its own alpha bytes alone (the test of the test)."""
    blocks, pool = blocks.cpu(), pool.cpu()
    clip = BS.pool_as_clip(blocks, pool, T, Hs, Ws, culled_rgba8)
    vis, dif, show, moves = texel_maps(clip)
    D, bh, bw = blocks.shape

    def block_any(m):
        m = torch.nn.functional.pad(m, (0, bw * 8 - Ws, 0, bh * 8 - Hs))      # texels past the plane never count
        return m.reshape(D, bh, 8, bw, 8).any(4).any(2)
    e = blocks.long()
    stored, dynamic = e >= 0, (e >= 0) & ((e & 1) == 1)
    culled_visible = BS.rgba8_bytes(culled_rgba8)[3] > 0
    dropped = stored & ~block_any(vis if own_alpha_only else show) & (not culled_visible)
    demoted = dynamic & ~dropped & ~block_any(moves)
    still_dyn = dynamic & ~dropped & ~demoted
    size = torch.where(still_dyn, T, 1) * (stored & ~dropped).long()
    flat = size.flatten()
    start = torch.cumsum(flat, 0) - flat
    table = torch.where(flat > 0, start * 2 + still_dyn.flatten().long(), torch.full_like(start, -1))
    n_slots = int(flat.sum())
    new_pool = torch.zeros((n_slots * 64, 4), dtype=torch.uint8)
    old = e.flatten()
    for i in (flat > 0).nonzero()[:, 0].tolist():
        n, src, dst = int(flat[i]), int(old[i]) >> 1, int(start[i])
        new_pool[dst * 64:(dst + n) * 64] = pool[src * 64:(src + n) * 64]
    table = table.reshape(D, bh, bw).to(torch.int32)
    keep = quad_keep.cpu().bool() & quad_any(vis, quad_keep.shape, tile)
    dyn = keep & quad_any(moves, quad_keep.shape, tile)
    # (pool_as_clip forms an index for entries -1 too, up to slot T - 1, before it discards the value: a pool of fewer slots is padded for it)
    padded = torch.cat([new_pool, torch.zeros((max(0, T - n_slots) * 64, 4), dtype=torch.uint8)])
    return types.SimpleNamespace(vis=vis, dif=dif, show=show, moves=moves, size=size, dropped=dropped, demoted=demoted, blocks=table, pool=new_pool,
                                 n_slots=n_slots, keep=keep, dyn=dyn, clip=BS.pool_as_clip(table, padded, T, Hs, Ws, culled_rgba8))
