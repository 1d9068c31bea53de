"""Every refusal of the two RGB-D entries (include/vl3d.h "RGB-D": vl3d_render_rgbd_baked, vl3d_render_rgbd_baked_pool), in the style of
disparity_models.refusal_rows.  The entries refuse before anything touches a device, so the pointers are placeholders nothing reads -- which is
why the rows do not run where a device exists (a refusal that went missing would launch a kernel on them); tests/test_gpu_rgbd.py calls the
same rows on real buffers there and checks that the outputs stay untouched.  No GPU."""
import pytest
import torch

ENTRIES = ["vl3d_render_rgbd_baked", "vl3d_render_rgbd_baked_pool"]
EINVAL, ELAUNCH = 1, 2
P = 64      # a non-null, 16-byte aligned placeholder
PLACEHOLDERS = dict(baked=P, blocks=P, pool=P, homos=P, rows=P, qk=P, cull=P, rgb=P, alpha=P, disp=P, frames=P, depth16=P, idx=P)

no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="placeholder addresses: a refusal that went missing would launch a kernel on them")


def refusal_desc(**fields):
    """D 2, 3 output frames, 8 x 8 texels, 4 x 6 pixels, the planar convention, u8 texels"""
    from videoloop3d_amd import _lib as L
    d = L.RenderDesc()
    d.D, d.T, d.Hs, d.Ws, d.H, d.W = 2, 3, 8, 8, 4, 6
    d.coord_mode, d.border_mode, d.act_order = L.COORD["affine"], L.BORDER["hardcut"], L.ACT_ORDER["post"]
    d.rgb_act = d.alpha_act = L.ACT["sigmoid"]
    d.stack_dtype = L.STACK_DTYPE["u8"]
    d.pixel_center, d.sx, d.sy = 0.5, 1.0, 1.0
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def refusal_rows():
    """[(id, entry, descriptor fields, argument overrides, a fragment of the message)], every row VL3D_EINVAL.  Overrides: a pointer name ->
    None (NULL) or ("+", bytes) (misaligned by so many bytes); frame0 / QH / QW; sel -> "run" | "path" | "times" | "both" | "neither" | "half"
    | "no_cams" | "times_reserved" | "times_no_cam"; sink -> "float" | "display"; channels; bg -> True (a host colour) | "nan"."""
    rows = []
    for e in ENTRIES:
        pool = e == ENTRIES[1]
        src = "pool" if pool else "baked"
        with_map = {} if pool else dict(qk="map")      # (the pool always carries its map)
        rows += [
            # the colour entry of the same source
            ("utils-mpi-coordinates", e, dict(coord_mode=0), {}, b"the planar MPV convention only"),
            ("zeros-border", e, dict(border_mode=0), {}, b"the planar MPV convention only"),
            ("uv-noise", e, dict(uv_noise_seed=5), {}, b"add_uv_noise is a training switch"),
            ("a-variant", e, dict(variant=1), {}, b"no kernel variants"),
            ("float-texels", e, dict(stack_dtype=0), {}, b"stack_dtype must be VL3D_U8"),
            ("no-frames", e, dict(T=0), {}, b"non-positive render dims"),
            ("a-plane-of-one-row", e, dict(Hs=1), {}, b"at least 2 x 2 texels"),
            ("null-" + src, e, {}, {src: None}, b"null pointer"),
            ("misaligned-" + src, e, {}, {src: ("+", 2)}, b"4-byte aligned"),
            ("null-homos", e, {}, dict(homos=None), b"null pointer"),
            ("run-past-the-clip", e, {}, dict(frame0=3), b"the run of frames leaves"),
            ("run-before-the-clip", e, {}, dict(frame0=-1), b"the run of frames leaves"),
            ("half-a-path", e, {}, dict(sel="half"), b"neither a run"),
            ("a-path-of-no-cameras", e, {}, dict(sel="no_cams"), b"n_cams must be in [1, 65535]"),
            ("times-reserved", e, {}, dict(sel="times_reserved"), b"sel->reserved must be 0"),
            ("times-without-cameras", e, {}, dict(sel="times_no_cam"), b"null pointer (sel->frame_cam"),
            ("grid-of-mixed-signs", e, {}, dict(with_map, QW=-2), b"bad quad grid"),
            ("tile-exact-grid-of-ragged-tiles", e, {}, dict(with_map, QH=-3, QW=-2), b"whole tiles"),
            ("map-without-cull-scratch", e, {}, dict(with_map, cull=None), b"vl3d_render_cull_scratch_bytes"),
            ("five-channels", e, {}, dict(sink="display", channels=5), b"channels must be 3 (RGB8) or 4 (RGBA8)"),
            ("misaligned-rgba8", e, {}, dict(sink="display", channels=4, frames=("+", 2)), b"RGBA8 frames must be 4-byte aligned"),
            ("a-nan-background", e, {}, dict(sink="display", bg="nan"), b"the background colour must be finite"),
            ("a-background-with-the-float-sink", e, {}, dict(bg=True), b"a background colour belongs to the display sink"),
            # the disparity entry of the same source
            ("129-planes", e, dict(D=129), {}, b"at most 128 planes"),
            ("null-rows", e, {}, dict(rows=None), b"null pointer"),
            ("misaligned-rows", e, {}, dict(rows=("+", 2)), b"4-byte aligned"),
            ("misaligned-homos", e, {}, dict(homos=("+", 2)), b"4-byte aligned"),
            # the selection and the sink of this entry
            ("both-selections", e, {}, dict(sel="both"), b"exactly one of sel"),
            ("no-selection", e, {}, dict(sel="neither"), b"exactly one of sel"),
            ("null-out", e, {}, dict(sink="null"), b"null pointer (out)"),
            ("both-sinks", e, {}, dict(sink="both"), b"out names both sinks"),
            ("disp-beside-the-display-sink", e, {}, dict(sink="display", disp=P), b"out names both sinks"),
            ("no-sink", e, {}, dict(sink="neither"), b"null pointer (out: rgb, alpha and disp, or frames and depth16)"),
            ("a-float-sink-without-disp", e, {}, dict(disp=None), b"the float sink needs disp"),
            ("a-float-sink-without-rgb", e, {}, dict(rgb=None), b"null pointer (out: rgb and alpha"),
            ("a-float-sink-without-alpha", e, {}, dict(alpha=None), b"null pointer (out: rgb and alpha"),
            ("misaligned-disp", e, {}, dict(disp=("+", 2)), b"rgb, alpha and disp must be 4-byte aligned"),
            ("a-display-sink-without-depth16", e, {}, dict(sink="display", depth16=None), b"the display sink needs depth16"),
            ("a-display-sink-without-frames", e, {}, dict(sink="display", frames=None), b"null pointer (frames)"),
            ("misaligned-depth16", e, {}, dict(sink="display", depth16=("+", 1)), b"depth16 must be 2-byte aligned"),
        ]
        if pool:
            rows += [("null-blocks", e, {}, dict(blocks=None), b"null pointer"),
                     ("null-map", e, {}, dict(qk=None), b"the quad map and vl3d_render_cull_scratch_bytes"),
                     ("a-cull-window", e, dict(cull_Hs=16, cull_Ws=16), {}, b"the pool holds whole planes")]
    return rows


def call_refusal(entry, desc, ptr, over):
    """the entry on the addresses `ptr` with a row's overrides: a clip of 5 frames, the run of desc.T = 3 from frame 1 into the float sink, a
    2 x 2 quad map where the row (or the pool) carries one -> (status, message)"""
    import ctypes as C
    from videoloop3d_amd import _lib as L
    a = dict(ptr, frame0=1, QH=2, QW=2, sel="run", sink="float", channels=3, bg=None)
    if entry != ENTRIES[1] and over.get("qk") != "map":
        a["qk"], a["cull"], a["QH"], a["QW"] = None, None, 0, 0
    sink_kind = over.get("sink", "float")
    for k, v in over.items():
        if v == "map" or k == "sink":
            continue
        a[k] = (ptr[k] + v[1]) if isinstance(v, tuple) else v
    run = L.BakedFrames(frame0=int(a["frame0"]))
    path = L.BakedFrames(frame0=0, n_cams=1, frame_cam=a["idx"], frame_t=a["idx"])
    times = L.BakedTimes(n_cams=1, frame_cam=a["idx"], frame_time=a["idx"])
    sel, tsel = run, None
    kind = a["sel"]
    if kind == "path":
        sel = path
    elif kind == "times":
        sel, tsel = None, times
    elif kind == "both":
        tsel = times
    elif kind == "neither":
        sel = None
    elif kind == "half":
        sel = L.BakedFrames(frame0=0, n_cams=1, frame_cam=a["idx"])
    elif kind == "no_cams":
        sel = L.BakedFrames(frame0=0, n_cams=0, frame_cam=a["idx"], frame_t=a["idx"])
    elif kind == "times_reserved":
        sel, tsel = None, L.BakedTimes(n_cams=1, reserved=1, frame_cam=a["idx"], frame_time=a["idx"])
    elif kind == "times_no_cam":
        sel, tsel = None, L.BakedTimes(n_cams=1, frame_time=a["idx"])
    bg = None
    if a["bg"] is not None:
        bg = (C.c_float * 3)(0.25, float("nan") if a["bg"] == "nan" else 0.5, 0.75)
    out = L.RgbdOut(channels=int(a["channels"]), bg=None if bg is None else C.addressof(bg))
    if sink_kind in ("float", "both"):
        out.rgb, out.alpha, out.disp = a["rgb"], a["alpha"], a["disp"]
    if sink_kind in ("display", "both"):
        out.frames, out.depth16 = a["frames"], a["depth16"]
        if sink_kind == "display" and "disp" in over:
            out.disp = a["disp"]
    out = None if sink_kind == "null" else out
    lib = L.lib()
    if entry == ENTRIES[0]:
        rc = lib.vl3d_render_rgbd_baked(desc, a["baked"], 5, a["homos"], a["rows"], sel, tsel, a["qk"], a["QH"], a["QW"], a["cull"], out, None)
    else:
        rc = lib.vl3d_render_rgbd_baked_pool(desc, a["blocks"], a["pool"], 5, a["homos"], a["rows"], sel, tsel, a["qk"], a["QH"], a["QW"], 0, a["cull"],
                                             out, None)
    return rc, lib.vl3d_last_error()


ROWS = [pytest.param(*r[1:], id=f"{r[1][12:]}-{r[0]}") for r in refusal_rows()]


@no_device
@pytest.mark.parametrize("entry, fields, over, fragment", ROWS)
def test_refusals_come_before_the_device(entry, fields, over, fragment):
    import __graft_entry__ as g
    g.build()
    rc, msg = call_refusal(entry, refusal_desc(**fields), PLACEHOLDERS, over)
    assert rc == EINVAL, (rc, msg)
    assert msg.startswith(entry.encode() + b": ") and fragment in msg, msg


@no_device
@pytest.mark.parametrize("sink", ["float", "display"])
@pytest.mark.parametrize("sel", ["run", "path", "times"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_the_rows_start_from_a_call_that_is_accepted(entry, sel, sink):
    """the placeholder call itself is refused by none of the rows, for every selection and sink: it reaches the launch, which fails without a
    device"""
    import __graft_entry__ as g
    g.build()
    rc, msg = call_refusal(entry, refusal_desc(), PLACEHOLDERS, dict(sel=sel, sink=sink))
    assert rc == ELAUNCH, (rc, msg)


def test_every_row_is_named_once():
    ids = [(r[1], r[0]) for r in refusal_rows()]
    assert len(set(ids)) == len(ids) and {e for e, _ in ids} == set(ENTRIES)
