"""The crop-aware optimiser's C ABI without a GPU: `vl3d_adam_window` has the layout csrc/vl3d_optim.hip asserts, the three window entries and
vl3d_render_bwd_adam refuse a malformed struct with a code and a message that names them, and the positional entries of before are gone.
The refusals come before anything touches a device, so the pointers are placeholders nothing reads -- which is why those tests do not run
where a device exists: a refusal that went missing would launch a kernel on them there, here it comes back as a HIP error code."""
import ctypes as C

import pytest
import torch

no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="placeholder addresses: a refusal that went missing would launch a kernel on them")
P = 64      # a non-null, aligned placeholder
D, T, Hs, Ws, WINDOW, H, W = 2, 3, 32, 40, (8, 8, 16, 24), 8, 12
ENTRIES = ("vl3d_adam_window_catchup", "vl3d_adam_window_step", "vl3d_adam_flush_older", "vl3d_render_bwd_adam")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from videoloop3d_amd import _lib
    _lib.lib()
    return _lib


def test_struct_layout_is_the_asserted_one(L):
    """the two literals of the static_asserts in csrc/vl3d_optim.hip"""
    assert C.sizeof(L.AdamWindow) == 152
    assert L.AdamWindow.blocks.offset == 144


def test_the_positional_entries_are_gone(L):
    lib = C.CDLL(L.LIB_PATH)
    for name in ("vl3d_adam_window_catchup_boxes", "vl3d_adam_window_step_boxes", "vl3d_adam_window_step_tail"):
        assert not hasattr(lib, name), name
    for name in ENTRIES[:3]:
        assert L.SIGNATURES[name][0][0] == C.POINTER(L.AdamWindow), name
    assert L.lib().vl3d_version() >= 101


def window(**over):
    """a struct every entry accepts (placeholders for the device pointers), then `over`"""
    from videoloop3d_amd import _lib
    aw = _lib.AdamWindow()
    aw.D, aw.T, aw.Hs, aw.Ws = D, T, Hs, Ws
    aw.y0, aw.x0, aw.wh, aw.ww = WINDOW
    aw.param = aw.exp_avg = aw.exp_avg_sq = aw.last_step = aw.hist = P
    aw.lr, aw.beta1, aw.beta2, aw.eps, aw.step = 1e-3, 0.9, 0.999, 1e-8, 1
    for k, v in over.items():
        setattr(aw, k, v)
    return aw


def call(L, entry, aw, min_depth=1):
    lib = L.lib()
    w = None if aw is None else C.byref(aw)
    if entry == "vl3d_adam_window_catchup":
        rc = lib.vl3d_adam_window_catchup(w, 0, P, 0.0, 0, None)
    elif entry == "vl3d_adam_window_step":
        rc = lib.vl3d_adam_window_step(w, P, 0, None)
    elif entry == "vl3d_adam_flush_older":
        rc = lib.vl3d_adam_flush_older(w, 1, min_depth, None)
    else:
        from videoloop3d_amd.render import RenderSpec, _desc_dims
        wh, ww = (WINDOW[2], WINDOW[3]) if aw is None else (aw.wh, aw.ww)
        desc = _desc_dims(D, T, wh, ww, H, W, RenderSpec.mpv(), 0)
        n = int(lib.vl3d_render_bwd_scratch_bytes(desc))
        rc = lib.vl3d_render_bwd_adam(desc, P, P, P, P, P, None, None, None, None, P, P, n, w, None)
    return rc, (lib.vl3d_last_error() or b"").decode()


# name -> (struct fields, the entries the refusal applies to); the flush does not read the window, only the step and the fused entry read `step`
ALL, WINDOWED = ENTRIES, (ENTRIES[0], ENTRIES[1], ENTRIES[3])
REFUSALS = {
    "D = 0": (dict(D=0), ALL),
    "window outside the plane": (dict(y0=24), WINDOWED),
    "y0 = 4": (dict(y0=4), WINDOWED),
    "window end neither aligned nor at the border": (dict(wh=12), WINDOWED),
    "blocks without quad maps": (dict(blocks=P), ALL),
    "quad grid with mixed signs": (dict(quad_keep=P, class_scratch=P, QH=4, QW=-5), ALL),
    "tile-exact grid that does not divide the plane": (dict(quad_keep=P, class_scratch=P, QH=-5, QW=-5), ALL),
    "null state pointer": (dict(exp_avg_sq=None), ALL),
    "step = 0": (dict(step=0), (ENTRIES[1], ENTRIES[3])),
}


@no_device
@pytest.mark.parametrize("entry", ENTRIES)
def test_null_struct_is_refused(L, entry):
    rc, msg = call(L, entry, None)
    assert rc != 0 and entry in msg, (rc, msg)


@no_device
@pytest.mark.parametrize("name", list(REFUSALS))
def test_malformed_struct_is_refused_by_every_entry_that_reads_it(L, name):
    over, entries = REFUSALS[name]
    for entry in entries:
        rc, msg = call(L, entry, window(**over))
        assert rc != 0 and entry in msg, (entry, rc, msg)


@no_device
def test_flush_refuses_min_depth_0(L):
    rc, msg = call(L, "vl3d_adam_flush_older", window(), min_depth=0)
    assert rc != 0 and "vl3d_adam_flush_older" in msg, (rc, msg)


@no_device
def test_fused_entry_refuses_a_window_that_is_not_the_descriptor_s(L):
    """vl3d_render_bwd_adam: adam->wh must be desc->Hs (the stack is the window's compact copy) -- a struct every other entry accepts"""
    from videoloop3d_amd.render import RenderSpec, _desc_dims
    lib = L.lib()
    desc = _desc_dims(D, T, WINDOW[2] + 8, WINDOW[3], H, W, RenderSpec.mpv(), 0)
    aw = window()
    rc = lib.vl3d_render_bwd_adam(desc, P, P, P, P, P, None, None, None, None, P, P, int(lib.vl3d_render_bwd_scratch_bytes(desc)), C.byref(aw), None)
    assert rc == 1 and "wh" in (lib.vl3d_last_error() or b"").decode()
