"""Video I/O on the MI355X (csrc/vl3d_video.hip, videoloop3d_amd/y4m.py; docs/kernels/K10_video_io.md).

  1  the kernels against the rule (y4m.rgb8_to_yuv8 / yuv8_to_rgb8 on the CPU), byte for byte, inside sentinel bytes that must survive: every
     shape of SHAPES x N x channels x chroma x siting x matrix x range x frame stride, tight odd-sized I420 frames (U / V at odd addresses);
     vl3d_video_choice asserted on every call, and the aligned shapes forced through the byte path too
  2  the kernels against the float64 definition (tests/video_statement.py)
  3  Y4MWriter in chunks of 1, 3 and all; the source overwritten right after every write
  4  Y4MReader ranges, both layouts, both sitings          5  write_video of the smallest baked model, integer and fractional times
  6  videos_from_y4m into evaluate_views and MVVidPatchDataset          7  the entries' refusals on real buffers: nothing is written
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import baked_models as BM  # noqa: E402
import video_statement as VS  # noqa: E402
from videoloop3d_amd import synth, y4m  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 2), (3, 5), (8, 64), (9, 65), (16, 128), (17, 130), (64, 256)]
COMBOS = [(m, fr) for m in ("bt601", "bt709") for fr in (False, True)]
SENT, PAD = 0xA5, 64


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as g
    g.build()
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def bytes_of(shape, seed):
    return (synth.hash_uniform(shape, seed=seed) * 256).clamp(0, 255).to(torch.uint8)


def expect_wide(H, W, chroma, stride, *addresses):
    return W % 16 == 0 and (chroma == "444" or H % 2 == 0) and stride % 16 == 0 and all(a % 16 == 0 for a in addresses)


def choice_of(N, H, W, channels, chroma, sink, y_ptr, stride, rgb_ptr, decode, path=0):
    return y4m.video_choice(y4m._desc(N, H, W, channels, chroma, "center", "bt601", False, sink, y_ptr, stride, path), rgb_ptr, decode)


def strides_of(fb):
    return [fb, (fb + 15) // 16 * 16 + 16, fb + 5]      # tight; wider and 16-byte aligned; wider and odd


def packed(planes, N, stride, chroma):
    """the rule's planes as the payload holds them: N frames `stride` apart, the gaps between frames filled with sentinels"""
    H, W = planes[0].shape[1:]
    buf = torch.full(((N - 1) * stride + y4m.frame_bytes(H, W, chroma),), SENT, dtype=torch.uint8)
    for dst, src in zip(y4m.planes_of(buf, N, H, W, chroma, stride), planes):
        dst.copy_(src)
    return buf


# ---- 1. the kernels against the rule -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
def test_encode_stores_the_rules_bytes(dev, H, W):
    seen = set()
    for N in (1, 3):
        for channels in (3, 4):
            frames = bytes_of((N, H, W, channels), seed=H * 1000 + W + N + channels)
            fd = frames.to(dev)
            for chroma in ("444", "420"):
                fb = y4m.frame_bytes(H, W, chroma)
                for (matrix, full_range), stride in zip(COMBOS * 2, strides_of(fb) * 3):
                    want = packed(y4m.rgb8_to_yuv8(frames, chroma, matrix, full_range), N, stride, chroma)
                    n = (N - 1) * stride + fb
                    for path in (0, 1):
                        big = torch.full((n + 2 * PAD,), SENT, dtype=torch.uint8, device=dev)
                        buf = big[PAD:PAD + n]
                        took = choice_of(N, H, W, channels, chroma, "u8", buf.data_ptr(), stride, fd.data_ptr(), False, path)
                        assert took == ("wide" if path == 0 and expect_wide(H, W, chroma, stride, buf.data_ptr(), fd.data_ptr()) else "byte")
                        seen.add(took)
                        y4m.encode_frames(fd, buf, stride=stride, chroma=chroma, matrix=matrix, full_range=full_range, path=path)
                        got = big.cpu()
                        assert torch.equal(got[PAD:PAD + n], want), (N, channels, chroma, matrix, full_range, stride, took)
                        assert bool((got[:PAD] == SENT).all()) and bool((got[PAD + n:] == SENT).all())
    assert seen == ({"wide", "byte"} if W % 16 == 0 and H % 2 == 0 else {"byte"})


@pytest.mark.parametrize("layout", ["u8", "float"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_decode_stores_the_rules_bytes(dev, H, W, layout):
    took_all = set()
    for N in (1, 3):
        for chroma, siting in (("444", "center"), ("420", "center"), ("420", "left")):
            ch, cw = y4m.chroma_size(H, W, chroma)
            fb = y4m.frame_bytes(H, W, chroma)
            planes = (bytes_of((N, H, W), 1 + N), bytes_of((N, ch, cw), 2 + N), bytes_of((N, ch, cw), 3 + N))
            for (matrix, full_range), stride in zip(COMBOS * 2, strides_of(fb) * 3):
                src = packed(planes, N, stride, chroma).to(dev)
                for channels in ((3, 4) if layout == "u8" else (3,)):
                    want = y4m.yuv8_to_rgb8(*planes, chroma, siting, matrix, full_range, layout)
                    if channels == 4:
                        want = torch.cat([want, torch.full((N, H, W, 1), 255, dtype=torch.uint8)], dim=-1)
                    for path, shift in ((0, 0), (1, 0), (0, 1)):      # auto; forced byte; an output one element off the alignment
                        if layout == "u8":
                            big = torch.full((want.numel() + 2 * PAD,), SENT, dtype=torch.uint8, device=dev)
                        else:
                            big = torch.full((want.numel() + 2 * PAD,), -7.0, dtype=torch.float32, device=dev)
                        out = big[PAD + shift:PAD + shift + want.numel()].view(want.shape)
                        took = choice_of(N, H, W, channels, chroma, layout, src.data_ptr(), stride, out.data_ptr(), True, path)
                        assert took == ("wide" if path == 0 and expect_wide(H, W, chroma, stride, src.data_ptr(), out.data_ptr()) else "byte")
                        took_all.add(took)
                        y4m.decode_frames(src, N, H, W, stride=stride, chroma=chroma, siting_x=siting, matrix=matrix, full_range=full_range,
                                          layout=layout, channels=channels, out=out, path=path)
                        got = big.cpu()
                        assert torch.equal(got[PAD + shift:PAD + shift + want.numel()].view(want.shape), want), (N, chroma, siting, matrix, full_range, stride, channels, took)
                        sent = SENT if layout == "u8" else -7.0
                        assert bool((got[:PAD + shift] == sent).all()) and bool((got[PAD + shift + want.numel():] == sent).all())
    assert took_all == ({"wide", "byte"} if W % 16 == 0 and H % 2 == 0 else {"byte"})


def test_tight_odd_i420_frames_put_chroma_at_odd_addresses(dev):
    N, H, W = 3, 3, 5      # 15 bytes of luma, 3 x 2 of each chroma plane: U at +15, V at +21, frames 27 bytes apart
    frames = bytes_of((N, H, W, 3), seed=77)
    buf = y4m.encode_frames(frames.to(dev), chroma="420", matrix="bt601")
    assert buf.numel() == 81 and (buf.data_ptr() + 15) % 2 == 1
    planes = y4m.rgb8_to_yuv8(frames, "420", "bt601")
    assert torch.equal(buf.cpu(), packed(planes, N, 27, "420"))
    for got, want in zip(y4m.planes_of(buf, N, H, W, "420"), planes):
        assert torch.equal(got.cpu(), want)
    assert torch.equal(y4m.decode_frames(buf, N, H, W, matrix="bt601").cpu(), y4m.yuv8_to_rgb8(*planes, "420", "center", "bt601"))


@pytest.mark.parametrize("path", [0, 1])
def test_the_float_sink_divides_every_byte_by_255(dev, path):
    """full range, neutral chroma: R = G = B = Y, so the 256 luma values reach the sink as all 256 bytes"""
    y = torch.arange(256, dtype=torch.uint8).reshape(1, 16, 16)
    c = torch.full((1, 16, 16), 128, dtype=torch.uint8)
    out = y4m.decode_frames(packed((y, c, c), 1, 768, "444").to(dev), 1, 16, 16, chroma="444", matrix="bt601", full_range=True, layout="float", path=path)
    want = (torch.arange(256, dtype=torch.float32) / 255).reshape(1, 1, 16, 16).expand(1, 3, 16, 16)
    assert torch.equal(out.cpu(), want)


# ---- 2. the kernels against the float64 definition -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix,full_range", COMBOS)
def test_kernels_against_the_float64_definition(dev, matrix, full_range):
    enc, dec = [], []
    for H, W in ((9, 65), (16, 128), (64, 256)):
        frames = bytes_of((2, H, W, 3), seed=H + W)
        for chroma in ("444", "420"):
            buf = y4m.encode_frames(frames.to(dev), chroma=chroma, matrix=matrix, full_range=full_range)
            delta = VS.encode_delta(y4m.encode_coefs(matrix, full_range)[0], matrix, full_range)
            vals = VS.encode_values(frames.numpy(), chroma, matrix, full_range)
            enc += [(p.cpu().numpy(), v, d) for p, v, d in zip(y4m.planes_of(buf, 2, H, W, chroma), vals, delta)]
            ch, cw = y4m.chroma_size(H, W, chroma)
            planes = (bytes_of((2, H, W), 5), bytes_of((2, ch, cw), 6), bytes_of((2, ch, cw), 7))
            fb = y4m.frame_bytes(H, W, chroma)
            for siting in (("center", "left") if chroma == "420" else ("center",)):
                got = y4m.decode_frames(packed(planes, 2, fb, chroma).to(dev), 2, H, W, chroma=chroma, siting_x=siting, matrix=matrix, full_range=full_range)
                dec.append((got.cpu().numpy(), VS.decode_values(*[p.numpy() for p in planes], chroma, siting, matrix, full_range),
                            VS.decode_delta(y4m.decode_coefs(matrix, full_range)[0], matrix, full_range)))
    VS.compare_pooled(enc, f"device encode {matrix} full={full_range}")
    VS.compare_pooled(dec, f"device decode {matrix} full={full_range}")


# ---- 3. the writer ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chroma,H,W", [("420jpeg", 16, 32), ("420jpeg", 9, 13), ("444", 5, 16)])
def test_writer_chunks_write_the_same_file(dev, tmp_path, chroma, H, W):
    n = 7
    frames = bytes_of((n, H, W, 3), seed=21)
    c = "444" if chroma == "444" else "420"
    planes = y4m.rgb8_to_yuv8(frames, c, "bt601", False)
    want = f"YUV4MPEG2 W{W} H{H} F25:1 Ip A1:1 C{chroma} XCOLORRANGE=LIMITED\n".encode() \
        + b"".join(b"FRAME\n" + b"".join(p[i].numpy().tobytes() for p in planes) for i in range(n))
    for chunk in (1, 3, n):
        path = str(tmp_path / f"c{chunk}.y4m")
        with y4m.Y4MWriter(path, W, H, chroma=chroma, chunk=chunk) as w:
            for i0, i1 in ((0, 2), (2, 3), (3, 7)):
                src = frames[i0:i1].to(dev)
                w.write(src)
                src.fill_(0)      # ordered after the conversion on the same stream: the file must not see it
        assert w.frames_written == n and open(path, "rb").read() == want, chunk


# ---- 4. the reader ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctag,H,W", [("420jpeg", 16, 32), ("420mpeg2", 7, 9), ("444", 6, 16)])
def test_reader_ranges_decode_to_the_rule(dev, tmp_path, ctag, H, W):
    n = 9
    chroma, siting = y4m._CTAGS[ctag]
    ch, cw = y4m.chroma_size(H, W, chroma)
    planes = (bytes_of((n, H, W), 31), bytes_of((n, ch, cw), 32), bytes_of((n, ch, cw), 33))
    path = str(tmp_path / "r.y4m")
    with open(path, "wb") as f:
        f.write(f"YUV4MPEG2 W{W} H{H} F30:1 Ip C{ctag} XCOLORRANGE=FULL\n".encode())
        for i in range(n):
            f.write(b"FRAME\n" + b"".join(p[i].numpy().tobytes() for p in planes))
    want = y4m.yuv8_to_rgb8(*planes, chroma, siting, "bt709", True)
    for chunk in (1, 4, 16):
        r = y4m.Y4MReader(path, chunk=chunk)
        assert len(r) == n and (r.header.chroma, r.header.siting_x, r.header.full_range) == (chroma, siting, True)
        assert torch.equal(r.frames(dev, matrix="bt709").cpu(), want)
        assert torch.equal(r.frames(dev, start=1, count=4, step=2, matrix="bt709").cpu(), want[1:9:2])
        assert torch.equal(r.frames(dev, start=5, matrix="bt709").cpu(), want[5:])
    fl = y4m.load_clip(path, dev, start=2, count=3, layout="float", matrix="bt709", chunk=2)
    assert torch.equal(fl.cpu(), want[2:5].permute(0, 3, 1, 2).to(torch.float32) / 255)
    assert torch.equal(y4m.load_clip(path, dev).cpu(), y4m.yuv8_to_rgb8(*planes, chroma, siting, "bt601", True))      # auto: H < 720


# ---- 5. write_video ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fractional", [False, True])
def test_write_video_writes_the_rule_of_render_display(dev, tmp_path, fractional):
    from videoloop3d_amd import render_video as RV
    from videoloop3d_amd.baked import bake
    model, Hm, Wm, K = BM.tile_exact_model(dev, "0.2#0.4#0.6")
    baked = bake(model)
    n = 7
    ext = np.tile(np.eye(4, dtype=np.float32)[None], (n, 1, 1))
    for i in range(n):
        ext[i, :3, 3] = [0.03 * np.cos(i), 0.02 * np.sin(i), 0.004 * i]
    intr = np.tile(K.astype(np.float32)[None], (n, 1, 1))
    ts = RV.retime(n, 60, 25) if fractional else np.arange(n) % baked.frm_num
    path = str(tmp_path / "v.y4m")
    fps = 60 if fractional else 25
    assert RV.write_video(path, model, Hm, Wm, ext, intr, ts, fps=fps, baked=baked, fractional=fractional, max_batch=3) == n
    frames = baked.render_display(Hm, Wm, ext, intr, ts, fractional=fractional).cpu()
    assert float(frames.float().std()) > 1.0
    planes = y4m.rgb8_to_yuv8(frames, "420", "auto", False)
    r = y4m.Y4MReader(path)
    assert len(r) == n and r.header.fps == (fps, 1) and (r.header.W, r.header.H, r.header.ctag) == (Wm, Hm, "420jpeg")
    raw = open(path, "rb").read()
    assert raw == y4m.format_header(r.header) + b"".join(b"FRAME\n" + b"".join(p[i].numpy().tobytes() for p in planes) for i in range(n))
    assert torch.equal(r.frames(dev).cpu(), y4m.yuv8_to_rgb8(*planes, "420", "center", "auto", False))


# ---- 6. clips from files into the evaluation and the training set ------------------------------------------------------------------------------
def _model_of_frames(dev, T):
    """tests/baked_models.py: pool_model (tile-exact) with a clip of T frames -- the evaluation's first patch configuration takes temporal
    patches of 7 frames, which the 6-frame models do not hold"""
    import types
    from videoloop3d_amd import tiles
    from videoloop3d_amd.MPV import MPMeshVid
    model, Hm, Wm, K = BM.pool_model(torch.device("cpu"), "")
    args = types.SimpleNamespace(**dict(vars(model.args), mpv_frm_num=T))
    qh, qw, th, tw = 4, 6, 8, 8
    big = MPMeshVid(args, Hm, Wm, np.eye(4), K, 1.0, 100.0)
    stack = synth.make_plane_stack(model.mpi_d, T, qh * th, qw * tw, seed=5, alpha_bias=0.0) * 0.8
    keep, dyn = model.quad_keep.cpu(), model.quad_dyn.cpu()
    stack = torch.where(tiles.quad_to_texel_mask(dyn, qh * th, qw * tw, (th, tw))[:, None, :, :, None], stack, stack[:, :1])
    stack = torch.where(tiles.quad_to_texel_mask(keep, qh * th, qw * tw, (th, tw))[:, None, :, :, None], stack, torch.tensor([0.0, 0.0, 0.0, tiles.CULLED_ALPHA]))
    big.init_from_mpi({"ref_extrin": big.ref_extrin, "ref_intrin": big.ref_intrin, "planedepth": big.planedepth, "stack": stack, "quad_keep": keep,
                       "quad_dyn": dyn, "self.is_sparse": True, "self.has_dyn": True, "self.tile_own": (th, tw), "self.tile_full": (th, tw)})
    return big.to(dev).eval(), K


def test_videos_from_y4m_feed_the_evaluation_and_the_dataset(dev, tmp_path):
    from videoloop3d_amd import evaluations as E
    from videoloop3d_amd.baked import bake
    from videoloop3d_amd.train_3dvid import MVVidPatchDataset
    T, H, W, crop = 8, 56, 72, 4
    model, K = _model_of_frames(dev, T)
    baked = bake(model)
    ext = np.eye(4, dtype=np.float32)[None]
    Ks = K.astype(np.float32)[None].copy()
    Ks[:, 0, 2] += (W - 64) / 2
    Ks[:, 1, 2] += (H - 36) / 2
    own = baked.render_display(H, W, torch.tensor(np.repeat(ext, T, 0)), torch.tensor(np.repeat(Ks, T, 0)), np.arange(T))
    noise = (synth.hash_uniform((T + 1, H, W, 3), 40, device=dev) * 11).long() - 5
    gt = (torch.cat([own, own[:1]]).long() + noise).clamp(0, 255).to(torch.uint8)
    paths = [str(tmp_path / f"gt{v}.y4m") for v in range(2)]
    for p in paths:
        with y4m.Y4MWriter(p, W, H, chroma="444", full_range=True) as w:
            w.write(gt)
    vids = y4m.videos_from_y4m(",".join(paths), dev)
    want = y4m.yuv8_to_rgb8(*y4m.rgb8_to_yuv8(gt.cpu(), "444", "auto", True), "444", "center", "auto", True)
    assert len(vids) == 2 and all(v.is_cuda and torch.equal(v.cpu(), want) for v in vids)
    assert int((want.long() - gt.cpu().long()).abs().max()) <= 2      # 4:4:4 full range: the file is the clip to a rounding or two
    res = E.evaluate_views(model, vids[:1], ext, Ks, crop=crop, baked=baked)
    assert res == E.evaluate_views(model, [want.numpy()], ext, Ks, crop=crop, baked=baked) and np.isfinite(res[0]["psnr"])
    fl = y4m.videos_from_y4m(paths, dev, layout="float")
    assert fl[0].shape == (T + 1, 3, H, W) and torch.equal(fl[0].cpu(), want.permute(0, 3, 1, 2).float() / 255)
    poses = torch.eye(4)[None, :3].repeat(2, 1, 1)
    Kt = torch.as_tensor(Ks).repeat(2, 1, 1)
    ds = MVVidPatchDataset((H, W), fl, (16, 16), (8, 16), poses, Kt, loss_configs=[{"a": 1}, {"a": 2}], prepare=False)
    w0, h0, pose, intrin, patch, cfg = ds[0]
    assert patch.shape == (T + 1, 3, 16, 16) and cfg == {"a": 1}


# ---- 7. refusals on the device -----------------------------------------------------------------------------------------------------------------
def test_entries_refuse_on_real_buffers_and_write_nothing(dev):
    from videoloop3d_amd import _lib
    N, H, W = 2, 16, 32
    fb = y4m.frame_bytes(H, W, "420")
    frames = torch.full((N, H, W, 3), 7, dtype=torch.uint8, device=dev)
    buf = torch.full((N * fb,), SENT, dtype=torch.uint8, device=dev)
    out = torch.full((N, H, W, 3), SENT, dtype=torch.uint8, device=dev)
    outf = torch.full((N * 3 * H * W + 1,), -7.0, dtype=torch.float32, device=dev)
    st = _lib.stream_ptr(dev)

    def desc(**kw):
        d = y4m._desc(N, H, W, 3, "420", "center", "bt601", False, kw.pop("sink", "u8"), buf.data_ptr(), fb, 0)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    rows = [(dict(N=0), "N, H and W"), (dict(W=0), "N, H and W"), (dict(channels=5), "channels"), (dict(chroma=7), "chroma"), (dict(siting_x=-1), "siting_x"),
            (dict(matrix=2), "matrix"), (dict(full_range=3), "full_range"), (dict(sink=9), "sink"), (dict(path=2), "path"),
            (dict(frame_stride=fb - 1), "frame_stride"), (dict(y=None), "null plane"), (dict(v=None), "null plane"), (dict(N=70000, H=256, W=256), "grid limit")]
    for kw, naming in rows:
        for call in (lambda d: _lib.lib().vl3d_rgb8_to_yuv8(C.byref(d), _lib.ptr(frames), st), lambda d: _lib.lib().vl3d_yuv8_to_rgb(C.byref(d), _lib.ptr(out), st)):
            d = desc()
            for k, v in kw.items():
                setattr(d, k, v)
            assert call(d) == 1 and naming in _lib.lib().vl3d_last_error().decode(), (kw, _lib.lib().vl3d_last_error())
    assert _lib.lib().vl3d_rgb8_to_yuv8(C.byref(desc()), None, st) == 1 and b"null rgb" in _lib.lib().vl3d_last_error()
    assert _lib.lib().vl3d_yuv8_to_rgb(C.byref(desc()), None, st) == 1 and b"null rgb" in _lib.lib().vl3d_last_error()
    assert _lib.lib().vl3d_yuv8_to_rgb(C.byref(desc(sink="float")), C.c_void_p(outf.data_ptr() + 2), st) == 1 and b"4-byte aligned" in _lib.lib().vl3d_last_error()
    assert _lib.lib().vl3d_yuv8_to_rgb(C.byref(desc(sink="float", channels=4)), _lib.ptr(outf), st) == 1
    with pytest.raises(ValueError, match="payload"):
        y4m.encode_frames(frames, buf[:-1])
    with pytest.raises(ValueError, match="payload"):
        y4m.decode_frames(buf, N, H, W, stride=fb - 1)
    with pytest.raises(RuntimeError, match="path"):
        y4m.encode_frames(frames, buf, path=5)
    torch.cuda.synchronize()
    assert bool((buf == SENT).all()) and bool((out == SENT).all()) and bool((outf == -7.0).all())      # nothing was launched
