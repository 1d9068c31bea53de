"""Fractional loop time of the baked playback model, off the device: the reduction of real playback times into the loop (baked.loop_times), the
retiming of a loop to another display rate (render_video.retime), the selection struct vl3d_baked_times with its two entries (header, library,
binding) and what they refuse, and render_frames(fractional=True) without a baked model.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["vl3d_render_fwd_baked_times", "vl3d_render_fwd_baked_pool_times"]


# ---- 1. loop_times -------------------------------------------------------------------------------------------------------------------------
def test_loop_times_reduces_into_the_loop():
    from videoloop3d_amd.baked import loop_times
    got = loop_times([0, 4.75, 5.0, 7.5, -0.25, -5.0, -1e-9], 5)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32
    assert got.tolist() == [0, 4.75, 0, 2.5, 4.75, 0, 0]
    assert np.signbit(got).sum() == 0                                            # no -0.0 either: the kernel compares, but keep them plain
    # every value is below T after the cast, whatever goes in: times just below a multiple of T, large times, a numpy array, T = 1
    rng = np.random.default_rng(5)
    for T in (1, 2, 5, 50, 60):
        t = np.concatenate([rng.uniform(-1e6, 1e6, 4096), np.arange(-3, 4) * T - 1e-9, np.arange(-3, 4) * T - 1e-5, np.nextafter(np.arange(1, 4) * float(T), 0)])
        r = loop_times(t, T)
        assert r.dtype == np.float32 and r.shape == t.shape and bool((r >= 0).all()) and bool((r < T).all())
        # ... and is the float64 reduction, up to the cast and the wrap of a value that rounds to T
        want = t - T * np.floor(t / T)
        d = np.abs(r.astype(np.float64) - want)
        assert float(np.minimum(d, T - d).max()) <= T * 2.0 ** -24
    assert loop_times(3, 5).tolist() == [3.0]                                    # a scalar is a path of one
    assert loop_times([], 5).shape == (0,)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="finite"):
            loop_times([0.5, bad], 5)
    with pytest.raises(ValueError):
        loop_times([0.5], 0)


# ---- 2. retime -----------------------------------------------------------------------------------------------------------------------------
def test_retime_gives_unreduced_loop_times():
    from videoloop3d_amd.baked import loop_times
    from videoloop3d_amd.render_video import retime
    t = retime(6, 60, 25)
    assert t.dtype == np.float64 and np.array_equal(t, np.arange(6) * 25.0 / 60.0)
    assert np.array_equal(retime(6, 60), t)                                      # the loop's own rate is the reference's 25 fps
    # reduced at T = 2 the loop wraps between output frames 4 (1.667) and 5 (2.083 -> 0.083)
    r = loop_times(t, 2)
    assert np.array_equal(r, (t - 2 * np.floor(t / 2)).astype(np.float32))
    assert np.floor(r).tolist() == [0, 0, 0, 1, 1, 0] and abs(float(r[5]) - (125.0 / 60.0 - 2.0)) < 1e-6
    # half speed doubles the output frames per loop frame; the display rate of the loop itself is the identity
    assert np.array_equal(retime(5, 60, 25, speed=0.5), np.arange(5) * 12.5 / 60.0)
    assert np.array_equal(retime(7, 25, 25), np.arange(7, dtype=np.float64))
    assert np.array_equal(loop_times(retime(4, 25, 25, speed=-1.0), 5), np.array([0, 4, 3, 2], dtype=np.float32))
    with pytest.raises(ValueError):
        retime(4, 0)


# ---- 3. the struct and the two entries, by name --------------------------------------------------------------------------------------------
def test_times_entries_take_their_selection_and_the_sink_struct():
    import __graft_entry__ as g
    g.build()
    from videoloop3d_amd import _lib as L
    assert ctypes.sizeof(L.BakedTimes) == 24
    assert [f[0] for f in L.BakedTimes._fields_] == ["n_cams", "reserved", "frame_cam", "frame_time"]
    assert ctypes.sizeof(L.BakedFrames) == 24 and [f[0] for f in L.BakedFrames._fields_] == ["frame0", "n_cams", "frame_cam", "frame_t"]      # untouched
    raw = open(os.path.join(ROOT, "include", "vl3d.h")).read()
    body = re.search(r"typedef struct vl3d_baked_times \{(.*?)\} vl3d_baked_times;", raw, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()]
    assert decls == ["int32_t n_cams", "int32_t reserved", "const int32_t *frame_cam", "const float *frame_time"]
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in include/vl3d.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        argtypes, restype = L.SIGNATURES[name]
        assert restype is ctypes.c_int and argtypes[-2] is ctypes.POINTER(L.BakedOut) and argtypes.count(ctypes.POINTER(L.BakedTimes)) == 1
        assert argtypes.count(ctypes.POINTER(L.BakedFrames)) == 0
        decl = re.sub(r"\s+", " ", re.search(name + r"\s*\(([^;]*)\)\s*;", header).group(1))
        assert "const vl3d_baked_times *sel" in decl and "const vl3d_baked_out *out" in decl
        assert "float *rgb" not in decl and "uint8_t *frames" not in decl and "frame_time" not in decl
        # ... and otherwise the argument list of the entry it stands beside
        assert argtypes == [ctypes.POINTER(L.BakedTimes) if a is ctypes.POINTER(L.BakedFrames) else a for a in L.SIGNATURES[name[:-len("_times")]][0]]


@pytest.mark.parametrize("entry", ENTRIES)
def test_times_selection_and_sink_refusals(entry):
    """a `sel` with a NULL pointer, a set reserved field or n_cams out of range, an `out` that names both sinks or neither, a background with the
    float sink: VL3D_EINVAL with a message of its own, from either entry.  The refusals come before anything touches a device: the pointers are
    placeholders nothing reads."""
    import __graft_entry__ as g
    g.build()
    from videoloop3d_amd import _lib as L
    lib = L.lib()
    d = L.RenderDesc()
    d.D, d.T, d.Hs, d.Ws, d.H, d.W = 2, 3, 8, 8, 4, 6
    d.coord_mode, d.border_mode, d.stack_dtype = L.COORD["affine"], L.BORDER["hardcut"], L.STACK_DTYPE["u8"]
    p = 64      # a non-null, aligned placeholder
    bg = (ctypes.c_float * 3)(0.2, 0.4, 0.6)
    ok, fl = L.BakedTimes(n_cams=1, frame_cam=p, frame_time=p), L.BakedOut(rgb=p, alpha=p)

    def call(sel, out, desc=d):
        if entry == "vl3d_render_fwd_baked_times":
            return lib.vl3d_render_fwd_baked_times(desc, p, 5, p, sel, p, 2, 2, p, out, None)
        return lib.vl3d_render_fwd_baked_pool_times(desc, p, p, 5, p, sel, p, 2, 2, 0, p, out, None)

    seen = set()

    def refused(fragment, sel, out, **kw):
        assert call(sel, out, **kw) == 1, fragment
        msg = lib.vl3d_last_error()
        assert msg.startswith(entry.encode() + b": ") and fragment in msg, msg
        seen.add(msg)
    refused(b"null pointer (sel->frame_time", L.BakedTimes(n_cams=1, frame_cam=p), fl)
    refused(b"null pointer (sel->frame_cam", L.BakedTimes(n_cams=1, frame_time=p), fl)
    refused(b"n_cams must be in [1, 65535]", L.BakedTimes(n_cams=0, frame_cam=p, frame_time=p), fl)
    assert len(seen) == 3
    refused(b"n_cams must be in [1, 65535]", L.BakedTimes(n_cams=65536, frame_cam=p, frame_time=p), fl)
    refused(b"reserved must be 0", L.BakedTimes(n_cams=1, reserved=1, frame_cam=p, frame_time=p), fl)
    refused(b"null pointer (sel)", None, fl)
    refused(b"both sinks", ok, L.BakedOut(rgb=p, alpha=p, frames=p, channels=3))
    refused(b"both sinks", ok, L.BakedOut(alpha=p, frames=p, channels=4))
    refused(b"null pointer (out", ok, L.BakedOut())
    refused(b"null pointer (out", ok, L.BakedOut(rgb=p))
    refused(b"null pointer (out)", ok, None)
    refused(b"background", ok, L.BakedOut(rgb=p, alpha=p, bg=ctypes.addressof(bg)))
    assert len(seen) == 9                                                        # every rule has a message of its own
    # the rules of the path form, with its messages: the display sink's, the descriptor's
    refused(b"channels must be 3", ok, L.BakedOut(frames=p, channels=2))
    f32 = L.RenderDesc.from_buffer_copy(d)
    f32.stack_dtype = L.STACK_DTYPE["f32"]
    refused(b"stack_dtype must be VL3D_U8", ok, fl, desc=f32)


# ---- 4. render_frames --------------------------------------------------------------------------------------------------------------------
def test_render_frames_retimes_the_baked_model_only():
    from videoloop3d_amd import render_video as RV

    class Model:
        training = False

        def eval(self):
            raise AssertionError("the float model is not touched")
    ext = np.tile(np.eye(4, dtype=np.float32)[None], (3, 1, 1))
    intr = np.tile(np.eye(3, dtype=np.float32)[None], (3, 1, 1))
    with pytest.raises(ValueError, match="baked="):
        RV.render_frames(Model(), 4, 6, ext, intr, RV.retime(3, 60), fractional=True)
    # with a baked model the times go to its render_display unreduced and unrounded, one pose per time
    calls = []

    class Baked:
        bg_color = ""

        def render_display(self, H, W, e, k, ts, **kw):
            calls.append((H, W, len(e), len(k), np.asarray(ts).tolist(), kw))
            return "frames"
    assert RV.render_frames(Model(), 4, 6, ext, intr, RV.retime(5, 60), max_batch=2, baked=Baked(), fractional=True) == "frames"
    assert calls == [(4, 6, 3, 3, (np.arange(3) * 25.0 / 60.0).tolist(), dict(channels=3, max_batch=2, fractional=True))]
