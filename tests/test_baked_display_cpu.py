"""The display output of the baked playback model, off the device: the display rule in torch (videoloop3d_amd/baked.display_frames) against
numpy statements of the reference's `to8b` and of its background composite, the two baked render entries with their selection and sink
structs (header, library, binding) and what they refuse about the two structs, and how `render_display` launches a selection -- `render_video.path_segments`: a chunk that is one run makes one run call, any other chunk one
path call, each carrying its uint8 slice of the result -- on a stubbed backend.  No GPU."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["vl3d_render_fwd_baked", "vl3d_render_fwd_baked_pool"]


# ---- 1. the display rule -------------------------------------------------------------------------------------------------------------------
def _values():
    """float32 values where truncation decides: 0, 1, every k / 255, the float just below and just above each, and values outside [0, 1]."""
    k = (np.arange(256, dtype=np.float64) / 255).astype(np.float32)
    below, above = np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2))
    outside = np.array([-1e30, -2.0, -0.5, -1e-30, -0.0, 1.0 + 1e-6, 1.5, 2.0, 255.0, 1e30], dtype=np.float32)
    return np.concatenate([k, below, above, outside])


def _np_to8b(x):
    return (255 * np.clip(x, 0, 1)).astype(np.uint8)      # utils.py: to8b


def test_display_frames_is_to8b():
    from videoloop3d_amd.baked import display_frames
    v = _values()
    n = len(v) // 3 * 3
    rgb = v[:n].reshape(1, 1, n // 3, 3)
    alpha = v[np.arange(n // 3) * 2 % len(v)].reshape(1, 1, n // 3)
    assert rgb.dtype == np.float32
    got = display_frames(torch.from_numpy(rgb), torch.from_numpy(alpha), None, 3)
    assert got.dtype == torch.uint8 and got.shape == (1, 1, n // 3, 3)
    assert np.array_equal(got.numpy(), _np_to8b(rgb))
    # the levels themselves: 255 * (k / 255) is k in float32 for every k, the float below it truncates to k - 1
    k = (np.arange(256, dtype=np.float64) / 255).astype(np.float32)
    lv = display_frames(torch.from_numpy(k.reshape(1, 1, 256, 1).repeat(3, -1)), torch.zeros(1, 1, 256), None, 3).numpy()[0, 0, :, 0]
    want = _np_to8b(k)
    assert np.array_equal(lv, want) and int(np.abs(want.astype(int) - np.arange(256)).max()) <= 1 and want[0] == 0 and want[255] == 255
    # RGBA8: the alpha byte is to8b of alpha
    got4 = display_frames(torch.from_numpy(rgb), torch.from_numpy(alpha), None, 4)
    assert got4.shape == (1, 1, n // 3, 4) and np.array_equal(got4[..., :3].numpy(), got.numpy())
    assert np.array_equal(got4[..., 3].numpy(), _np_to8b(alpha))
    with pytest.raises(ValueError, match="channels"):
        display_frames(torch.from_numpy(rgb), torch.from_numpy(alpha), None, 2)


@pytest.mark.parametrize("bg", [(1.0, 1.0, 1.0), (0.2, 0.4, 0.6), (2.0, -1.0, 0.5)])
def test_display_frames_over_a_background(bg):
    """the five-step expression in numpy float32, every step rounded on its own: m1 = c * A, o = (-A) + 1, m2 = bg * o, x = m1 + m2, to8b(x)"""
    from videoloop3d_amd.baked import display_frames
    v = _values()
    rng = np.random.default_rng(3)
    c = np.concatenate([v, rng.random(4096, dtype=np.float32)])
    A = np.concatenate([v[::-1], rng.random(4096, dtype=np.float32)])
    A[::7] = 1.0
    A[3::7] = 0.0
    rgb = np.stack([c, np.roll(c, 1), np.roll(c, 2)], -1).reshape(1, 1, -1, 3)
    alpha = A.reshape(1, 1, -1)
    b = np.asarray(bg, dtype=np.float32)
    m1 = rgb * alpha[..., None]
    o = (-alpha[..., None]) + np.float32(1)
    m2 = b[None, None, None] * o
    x = m1 + m2
    assert x.dtype == np.float32
    for channels in (3, 4):
        got = display_frames(torch.from_numpy(rgb), torch.from_numpy(alpha), bg, channels).numpy()
        assert np.array_equal(got[..., :3], _np_to8b(x))
        if channels == 4:
            assert np.array_equal(got[..., 3], _np_to8b(alpha))      # never composited
    # a tensor background gives the same bytes as the sequence
    assert torch.equal(display_frames(torch.from_numpy(rgb), torch.from_numpy(alpha), torch.tensor(bg), 3), torch.from_numpy(_np_to8b(x)))


# ---- 2. the entry points, by name ----------------------------------------------------------------------------------------------------------
def test_baked_entries_take_selection_and_sink_structs():
    import __graft_entry__ as g
    g.build()
    from videoloop3d_amd import _lib as L
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vl3d.h")).read(), flags=re.S)
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in include/vl3d.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        argtypes, restype = L.SIGNATURES[name]
        # (..., const vl3d_baked_out *out, stream), one selection struct in front of the quad map; no positional rgb / alpha / frames
        assert restype is ctypes.c_int and argtypes[-2] is ctypes.POINTER(L.BakedOut) and argtypes.count(ctypes.POINTER(L.BakedFrames)) == 1
        decl = re.sub(r"\s+", " ", re.search(name + r"\s*\(([^;]*)\)\s*;", header).group(1))
        assert "const vl3d_baked_frames *sel" in decl and "const vl3d_baked_out *out" in decl
        assert "float *rgb" not in decl and "uint8_t *frames" not in decl and "frame_cam" not in decl
    # the sink and the selection are fields: the display frames with their channel count and background, the path's cameras and indices
    assert [f[0] for f in L.BakedOut._fields_] == ["rgb", "alpha", "frames", "channels", "bg"]
    assert [f[0] for f in L.BakedFrames._fields_] == ["frame0", "n_cams", "frame_cam", "frame_t"]
    # the eight entries the two replace are gone from header, library and binding
    for old in ("_path", "_pool_path", "_u8", "_pool_u8", "_path_u8", "_pool_path_u8"):
        name = "vl3d_render_fwd_baked" + old
        assert name not in L.SIGNATURES and not hasattr(lib, name) and not re.search(r"\b" + name + r"\s*\(", header), name


@pytest.mark.parametrize("entry", ENTRIES)
def test_selection_and_sink_refusals(entry):
    """a `sel` that is neither a run nor a path, an `out` that names both sinks or neither, a background with the float sink: VL3D_EINVAL with a
    message of its own, from either entry.  The refusals come before anything touches a device: the pointers are placeholders nothing reads."""
    import __graft_entry__ as g
    g.build()
    from videoloop3d_amd import _lib as L
    lib = L.lib()
    d = L.RenderDesc()
    d.D, d.T, d.Hs, d.Ws, d.H, d.W = 2, 3, 8, 8, 4, 6
    d.coord_mode, d.border_mode, d.stack_dtype = L.COORD["affine"], L.BORDER["hardcut"], L.STACK_DTYPE["u8"]
    p = 64      # a non-null, aligned placeholder
    bg = (ctypes.c_float * 3)(0.2, 0.4, 0.6)
    run, fl = L.BakedFrames(frame0=1), L.BakedOut(rgb=p, alpha=p)

    def call(sel, out):
        if entry == "vl3d_render_fwd_baked":
            return lib.vl3d_render_fwd_baked(d, p, 5, p, sel, p, 2, 2, p, out, None)
        return lib.vl3d_render_fwd_baked_pool(d, p, p, 5, p, sel, p, 2, 2, 0, p, out, None)

    def refused(fragment, sel, out):
        assert call(sel, out) == 1, fragment
        msg = lib.vl3d_last_error()
        assert msg.startswith(entry.encode() + b": ") and fragment in msg, msg
    for sel in (L.BakedFrames(frame_cam=p), L.BakedFrames(frame_t=p), L.BakedFrames(n_cams=2), L.BakedFrames(n_cams=1, frame_cam=p)):
        refused(b"neither a run", sel, fl)
    refused(b"both sinks", run, L.BakedOut(rgb=p, alpha=p, frames=p, channels=3))
    refused(b"both sinks", run, L.BakedOut(alpha=p, frames=p, channels=4))
    refused(b"null pointer (out", run, L.BakedOut())
    refused(b"null pointer (out", run, L.BakedOut(rgb=p))
    refused(b"null pointer (out", run, L.BakedOut(channels=3, bg=ctypes.addressof(bg)))
    refused(b"background", run, L.BakedOut(rgb=p, alpha=p, bg=ctypes.addressof(bg)))
    refused(b"null pointer (sel)", None, fl)
    refused(b"null pointer (out)", run, None)
    # the refusals a path had before it was a struct keep their text
    refused(b"n_cams must be in [1, 65535]", L.BakedFrames(n_cams=0, frame_cam=p, frame_t=p), fl)
    refused(b"n_cams must be in [1, 65535]", L.BakedFrames(n_cams=65536, frame_cam=p, frame_t=p), fl)
    refused(b"leaves the", L.BakedFrames(frame0=3), fl)      # frames 3 .. 5 of 5


# ---- 3. how render_display launches a selection --------------------------------------------------------------------------------------------
def _stub(bg_color="0.25#0.5#1", T=5):
    """a _Baked whose backend records its calls: cameras by their intrinsics' [0, 0] entry, D = 2 planes"""
    from videoloop3d_amd.baked import _Baked
    calls = []

    class Stub(_Baked):
        device = torch.device("cpu")
        frm_num = T

        def _run(self, frame0, n, homos, H, W, out, **display):
            calls.append(("run", frame0, n, tuple(homos.shape), out, display))

        def _path(self, frame_cam, frame_t, homos, H, W, out, cull_scratch=None, **display):
            calls.append(("path", list(frame_cam), list(frame_t), tuple(homos.shape), out, display))
    s = Stub()
    s.bg_color = bg_color
    s.camera = types.SimpleNamespace(plane_homographies=lambda e, k: k[0, 0, 0] * torch.ones(2, 3, 3), _on=lambda device, name: torch.eye(4))
    return s, calls


def _poses(cams):
    ext = torch.eye(4)[None].repeat(len(cams), 1, 1)
    intr = torch.eye(3)[None].repeat(len(cams), 1, 1)
    intr[:, 0, 0] = torch.tensor(cams, dtype=torch.float32)
    return ext, intr


def _slice_of(view, base, c0, c1):
    return view.dtype == torch.uint8 and view.data_ptr() == base[c0:c1].data_ptr() and tuple(view.shape) == tuple(base[c0:c1].shape)


@pytest.mark.parametrize("channels", [3, 4])
def test_render_display_routing(channels):
    H, W = 4, 6
    s, calls = _stub()
    # a spiral of 7 poses over a clip of 5, chunks of 3: two path calls and a run of one frame
    ext, intr = _poses([10, 11, 12, 13, 14, 15, 16])
    ts = [0, 1, 2, 3, 4, 0, 1]
    out = s.render_display(H, W, ext, intr, ts, channels=channels, max_batch=3)
    assert out.dtype == torch.uint8 and out.shape == (7, H, W, channels)
    assert [c[0] for c in calls] == ["path", "path", "run"]
    assert calls[0][1:4] == ([0, 1, 2], [0, 1, 2], (3, 2, 3, 3)) and calls[1][1:4] == ([0, 1, 2], [3, 4, 0], (3, 2, 3, 3))
    assert calls[2][1:4] == (1, 1, (2, 3, 3))
    for (c0, c1), call in zip([(0, 3), (3, 6), (6, 7)], calls):
        assert call[4] is None                                             # no float output
        assert set(call[5]) == {"frames8", "bg"} and call[5]["bg"] == [0.25, 0.5, 1.0]
        assert _slice_of(call[5]["frames8"], out, c0, c1)
    # one chunk: one path call for the whole selection, into the caller's buffer
    del calls[:]
    buf = torch.zeros((7, H, W, channels), dtype=torch.uint8)
    assert s.render_display(H, W, ext, intr, ts, channels=channels, out=buf) is buf
    assert [c[0] for c in calls] == ["path"] and _slice_of(calls[0][5]["frames8"], buf, 0, 7)
    # a fixed view: runs (one per chunk), the camera's homographies, no path call
    del calls[:]
    ext, intr = _poses([3] * 5)
    out = s.render_display(H, W, ext, intr, [0, 1, 2, 3, 4], channels=channels, max_batch=2)
    assert [(c[0], c[1], c[2]) for c in calls] == [("run", 0, 2), ("run", 2, 2), ("run", 4, 1)]
    assert all(_slice_of(c[5]["frames8"], out, c0, c1) for c, (c0, c1) in zip(calls, [(0, 2), (2, 4), (4, 5)]))
    # a repeated camera and a break in the frame order inside a chunk: a path call whose cameras are numbered from the chunk's first
    del calls[:]
    ext, intr = _poses([5, 5, 6, 5])
    s.render_display(H, W, ext, intr, [1, 2, 3, 0], channels=channels)
    assert [c[0] for c in calls] == ["path"] and calls[0][1:4] == ([0, 0, 1, 0], [1, 2, 3, 0], (2, 2, 3, 3))


def test_render_display_refusals():
    H, W = 4, 6
    ext, intr = _poses([1, 1])
    s, calls = _stub("random")
    with pytest.raises(RuntimeError, match="render"):
        s.render_display(H, W, ext, intr, [0, 1])
    s, calls = _stub("")
    s.render_display(H, W, ext, intr, [0, 1])
    assert calls[0][5]["bg"] is None                                       # no background colour: none passed on
    with pytest.raises(IndexError):
        s.render_display(H, W, ext, intr, [4, 5])                          # a run that leaves the clip of 5
    with pytest.raises(ValueError, match="channels"):
        s.render_display(H, W, ext, intr, [0, 1], channels=2)
    with pytest.raises(RuntimeError, match="one pose"):
        s.render_display(H, W, ext, intr, [0, 1, 2])
    with pytest.raises(RuntimeError, match="`out`"):
        s.render_display(H, W, ext, intr, [0, 1], out=torch.zeros((2, H, W, 3)))
    assert s.render_display(H, W, ext[:0], intr[:0], []).shape == (0, H, W, 3)
