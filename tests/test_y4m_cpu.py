"""Video I/O off the device: the integer rule of videoloop3d_amd.y4m against the float64 definition of tests/video_statement.py (exhaustively
at 4:4:4, on hash-uniform frames at 4:2:0), the conditions that make that comparison a test (planted faults fail it), the .y4m container
(header, refusals, FRAME parameters, truncation, ranges, a writer / reader round trip through the rule), and the C side without a device:
the library's coefficient table, the choice function, and the entries' refusals on placeholder addresses.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import video_statement as VS  # noqa: E402
from videoloop3d_amd import synth, y4m  # noqa: E402

COMBOS = [(m, fr) for m in ("bt601", "bt709") for fr in (False, True)]
SIZES = [(1, 1), (2, 2), (3, 5), (8, 6), (9, 7)]


def frames_of(N, H, W, channels=3, seed=1):
    return (synth.hash_uniform((N, H, W, channels), seed=seed) * 256).clamp(0, 255).to(torch.uint8)


def encode_items(frames, chroma, matrix, full_range, got=None):
    """planes `got` (default: the rule's) beside the definition's values and the band: [(got, value, delta)] for video_statement.compare_pooled"""
    planes = got if got is not None else y4m.rgb8_to_yuv8(frames, chroma, matrix, full_range)
    delta = VS.encode_delta(y4m.encode_coefs(matrix, full_range)[0], matrix, full_range)
    vals = VS.encode_values(frames.numpy(), chroma, matrix, full_range)
    return [(p.numpy(), val, d) for p, val, d in zip(planes, vals, delta)]


def decode_items(y, u, v, chroma, siting_x, matrix, full_range, got=None):
    rgb = got if got is not None else y4m.yuv8_to_rgb8(y, u, v, chroma, siting_x, matrix, full_range)
    delta = VS.decode_delta(y4m.decode_coefs(matrix, full_range)[0], matrix, full_range)
    return [(rgb.numpy(), VS.decode_values(y.numpy(), u.numpy(), v.numpy(), chroma, siting_x, matrix, full_range), delta)]


def check_encode(frames, chroma, matrix, full_range, got=None, what=""):
    return VS.compare_pooled(encode_items(frames, chroma, matrix, full_range, got), f"encode {chroma} {matrix} {'full' if full_range else 'limited'} {what}")[0]


def check_decode(y, u, v, chroma, siting_x, matrix, full_range, got=None, what=""):
    return VS.compare_pooled(decode_items(y, u, v, chroma, siting_x, matrix, full_range, got),
                             f"decode {chroma} {siting_x} {matrix} {'full' if full_range else 'limited'} {what}")[0]


# ---- the rule against the definition ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix,full_range", COMBOS)
def test_rule_equals_definition_on_every_triple_444(matrix, full_range):
    """all 2^24 triples, both directions: RGB -> Y'CbCr and Y'CbCr -> RGB (every byte triple is a legal input of the decode)"""
    g = torch.arange(256, dtype=torch.uint8)
    for a0 in range(0, 256, 64):
        a = torch.arange(a0, a0 + 64, dtype=torch.uint8)
        cube = torch.stack(torch.meshgrid(a, g, g, indexing="ij"), dim=-1)      # [64,256,256,3]
        assert check_encode(cube, "444", matrix, full_range, what=f"slab {a0}") <= VS.BAND_CAP
        assert check_decode(cube[..., 0], cube[..., 1], cube[..., 2], "444", "center", matrix, full_range, what=f"slab {a0}") <= VS.BAND_CAP


@pytest.mark.parametrize("matrix,full_range", COMBOS)
def test_rule_equals_definition_420(matrix, full_range):
    """hash-uniform frames of odd and even sizes, both sitings; the sizes of a case are one population"""
    enc, dec = [], {"center": [], "left": []}
    for H, W in SIZES + [(32, 48), (33, 47)]:
        frames = frames_of(3, H, W, seed=H * 100 + W)
        enc += encode_items(frames, "420", matrix, full_range)
        ch, cw = y4m.chroma_size(H, W, "420")
        y, u, v = frames_of(3, H, W, 1, seed=7)[..., 0], frames_of(3, ch, cw, 1, seed=8)[..., 0], frames_of(3, ch, cw, 1, seed=9)[..., 0]
        for siting in dec:
            dec[siting] += decode_items(y, u, v, "420", siting, matrix, full_range)
    VS.compare_pooled(enc, f"encode 420 {matrix} full={full_range}")
    for siting, items in dec.items():
        VS.compare_pooled(items, f"decode 420 {siting} {matrix} full={full_range}")


@pytest.mark.parametrize("matrix,full_range", COMBOS)
@pytest.mark.parametrize("chroma", ["444", "420"])
def test_greys_black_white(chroma, matrix, full_range):
    g = torch.arange(256, dtype=torch.uint8).reshape(1, 16, 16, 1).expand(1, 16, 16, 3).contiguous()
    y, u, v = y4m.rgb8_to_yuv8(g, "444", matrix, full_range)
    assert (u == 128).all() and (v == 128).all(), "a grey has chroma exactly 128"
    assert (int(y[0, 0, 0]), int(y[0, 15, 15])) == ((0, 255) if full_range else (16, 235))
    flat = torch.full((1, 5, 7, 3), 200, dtype=torch.uint8)
    y, u, v = y4m.rgb8_to_yuv8(flat, chroma, matrix, full_range)
    assert (u == 128).all() and (v == 128).all()
    back = y4m.yuv8_to_rgb8(y, u, v, chroma, "center", matrix, full_range)
    assert (back[..., 0] == back[..., 1]).all() and (back[..., 1] == back[..., 2]).all(), "neutral chroma decodes to a grey"
    assert (back.to(torch.int32) - 200).abs().max() <= 1
    lo, hi = (0, 255) if full_range else (16, 235)
    ends = y4m.yuv8_to_rgb8(torch.tensor([[[lo, hi]]], dtype=torch.uint8), torch.full((1, 1, 2), 128, dtype=torch.uint8),
                            torch.full((1, 1, 2), 128, dtype=torch.uint8), "444", "center", matrix, full_range)
    assert ends.reshape(2, 3).tolist() == [[0, 0, 0], [255, 255, 255]]


@pytest.mark.parametrize("matrix,full_range", COMBOS)
def test_int32_range_at_the_extremes(matrix, full_range):
    """every intermediate of both directions fits int32 -- and the decode scale is the largest power of two of which that is true"""
    lo, hi = y4m.decode_extremes(matrix, full_range)
    assert -2 ** 31 <= lo and hi < 2 ** 31
    Cm, off = y4m.encode_coefs(matrix, full_range)
    for i in range(3):
        for shift, top in ((16, 255), (18, 1020)):
            base = (off[i] << shift) + (1 << (shift - 1))
            assert base + sum(c * top for c in Cm[i] if c > 0) < 2 ** 31 and base + sum(c * top for c in Cm[i] if c < 0) >= -2 ** 31
    # the rule, run in int32 on the extreme inputs, equals the same formula in Python integers
    ext = torch.tensor([0, 255], dtype=torch.uint8)
    cube = torch.stack(torch.meshgrid(ext, ext, ext, indexing="ij"), dim=-1).reshape(1, 1, 8, 3)
    got = y4m.yuv8_to_rgb8(cube[..., 0], cube[..., 1], cube[..., 2], "444", "center", matrix, full_range).reshape(8, 3).tolist()
    D, y0 = y4m.decode_coefs(matrix, full_range)
    for (Y, U, V), rgb in zip(cube.reshape(8, 3).tolist(), got):
        assert rgb == [min(255, max(0, (cy * (Y - y0) + cu * (16 * U - 2048) + cv * (16 * V - 2048) + (1 << 20)) >> 21)) for cy, cu, cv in D]
    if matrix == "bt709" and not full_range:      # the widest combination: one more bit would not fit
        assert 2 * hi >= 2 ** 31


def test_encode_coefficients_are_repaired():
    for matrix, full_range in COMBOS:
        Cm, off = y4m.encode_coefs(matrix, full_range)
        assert sum(Cm[1]) == 0 and sum(Cm[2]) == 0
        assert sum(Cm[0]) == round((1.0 if full_range else 219 / 255) * 65536)
        assert float(VS.encode_delta(Cm, matrix, full_range).max()) <= 0.0044


def test_auto_matrix():
    assert y4m.resolve_matrix("auto", 719) == "bt601" and y4m.resolve_matrix("auto", 720) == "bt709"
    with pytest.raises(ValueError, match="matrix"):
        y4m.resolve_matrix("bt2020", 8)


# ---- planted faults: the comparison is a test ------------------------------------------------------------------------------------------------
def test_planted_faults_fail_the_comparison():
    frames = frames_of(2, 32, 48, seed=11)
    m, fr = "bt601", False
    Cm, off = y4m.encode_coefs(m, fr)
    x = frames.to(torch.int32)
    with pytest.raises(AssertionError):      # Kr and Kb swapped
        check_encode(frames, "444", m, fr, got=y4m.rgb8_to_yuv8(frames, "444", (0.114, 0.299), fr), what="[swapped Kr / Kb]")
    trunc = [((Cm[i][0] * x[..., 0] + Cm[i][1] * x[..., 1] + Cm[i][2] * x[..., 2] + (off[i] << 16)) >> 16).clamp(0, 255).to(torch.uint8) for i in range(3)]
    with pytest.raises(AssertionError):      # truncation instead of rounding
        check_encode(frames, "444", m, fr, got=trunc, what="[truncated]")
    y, u, v = y4m.rgb8_to_yuv8(frames, "444", m, fr)
    with pytest.raises(AssertionError):      # chroma taken from the top-left pixel of the block
        check_encode(frames, "420", m, fr, got=(y, u[:, ::2, ::2], v[:, ::2, ::2]), what="[top-left chroma]")
    y, u, v = y4m.rgb8_to_yuv8(frames, "420", m, fr)
    with pytest.raises(AssertionError):      # the left siting applied to a centre-sited file
        check_decode(y, u, v, "420", "center", m, fr, got=y4m.yuv8_to_rgb8(y, u, v, "420", "left", m, fr), what="[left siting]")
    with pytest.raises(AssertionError):      # limited range read as full
        check_decode(y, u, v, "420", "center", m, fr, got=y4m.yuv8_to_rgb8(y, u, v, "420", "center", m, True), what="[range]")
    with pytest.raises(AssertionError):      # a rounded mean instead of the four-sample sum
        xs = x[:, 0::2, 0::2] + x[:, 0::2, 1::2] + x[:, 1::2, 0::2] + x[:, 1::2, 1::2]
        mean = ((xs + 2) >> 2)
        bad = [((Cm[i][0] * mean[..., 0] + Cm[i][1] * mean[..., 1] + Cm[i][2] * mean[..., 2] + (off[i] << 16) + (1 << 15)) >> 16).clamp(0, 255).to(torch.uint8)
               for i in (1, 2)]
        check_encode(frames, "420", m, fr, got=(y, bad[0], bad[1]), what="[rounded mean]")
    check_encode(frames, "420", m, fr)       # ... and the rule itself passes on the same frames
    check_decode(y, u, v, "420", "center", m, fr)


# ---- the container --------------------------------------------------------------------------------------------------------------------------
def write_raw(path, header, frames, frame_line=b"FRAME\n"):
    with open(path, "wb") as f:
        f.write(header)
        for fr in frames:
            f.write(frame_line)
            f.write(fr)
    return str(path)


def test_header_round_trip(tmp_path):
    h = y4m.Y4MHeader(6, 4, (30000, 1001), "p", (1, 1), "420jpeg", "LIMITED")
    line = y4m.format_header(h)
    assert line == b"YUV4MPEG2 W6 H4 F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n"
    assert y4m.parse_header(line[:-1]) == h
    p = write_raw(tmp_path / "a.y4m", line, [bytes(36)] * 2)
    assert y4m.read_header(p) == h
    for ctag, (chroma, siting) in {"420jpeg": ("420", "center"), "420mpeg2": ("420", "left"), "420": ("420", "center"), "444": ("444", "center")}.items():
        g = y4m.parse_header(f"YUV4MPEG2 W6 H4 F25:1 C{ctag}".encode())
        assert (g.chroma, g.siting_x, g.interlace, g.colorrange, g.full_range) == (chroma, siting, None, None, False)
    bare = y4m.parse_header(b"YUV4MPEG2 H4 W6")
    assert (bare.chroma, bare.siting_x, bare.fps, bare.frame_bytes) == ("420", "center", (25, 1), 36)
    assert y4m.parse_header(b"YUV4MPEG2 W6 H4 XCOLORRANGE=FULL XYSCSS=420JPEG").full_range


@pytest.mark.parametrize("header,naming", [
    (b"YUV4MPEG2 W6 H4 C420paldv", "C420paldv"), (b"YUV4MPEG2 W6 H4 C422", "C422"), (b"YUV4MPEG2 W6 H4 C411", "C411"),
    (b"YUV4MPEG2 W6 H4 Cmono", "Cmono"), (b"YUV4MPEG2 W6 H4 C420p10", "C420p10"), (b"YUV4MPEG2 W6 H4 C444p12", "C444p12"),
    (b"YUV4MPEG2 W6 H4 C422p16", "C422p16"), (b"YUV4MPEG2 W6 H4 It", "It"), (b"YUV4MPEG2 W6 H4 Ib", "Ib"), (b"YUV4MPEG2 W6 H4 Im", "Im"),
    (b"YUV4MPEG2 H4 F25:1", "W tag"), (b"YUV4MPEG2 W6 F25:1", "H tag"), (b"YUV4MPEG W6 H4", "magic"), (b"RIFF....AVI ", "magic"),
])
def test_header_refusals_name_the_tag(tmp_path, header, naming):
    with pytest.raises(ValueError, match=naming):
        y4m.read_header(write_raw(tmp_path / "bad.y4m", header + b"\n", [bytes(36)]))


def test_frame_lines_with_parameters_and_truncation(tmp_path):
    H, W = 4, 6
    frames = frames_of(3, H, W, seed=3)
    planes = y4m.rgb8_to_yuv8(frames, "420", "bt601", False)
    payload = [b"".join(p[i].numpy().tobytes() for p in planes) for i in range(3)]
    p = write_raw(tmp_path / "p.y4m", b"YUV4MPEG2 W6 H4 F25:1 Ip C420jpeg\n", payload, frame_line=b"FRAME Ixyz Xanything=1\n")
    r = y4m.Y4MReader(p)
    assert len(r) == 3
    want = y4m.yuv8_to_rgb8(*planes, "420", "center", "bt601", False)
    assert torch.equal(r.frames("cpu"), want)
    whole = open(p, "rb").read()
    for cut, frame in ((len(whole) - 1, 2), (len(whole) - 36 - 3, 2), (len(whole) - 2 * (36 + 23) + 5, 1)):
        q = tmp_path / f"cut{cut}.y4m"
        q.write_bytes(whole[:cut])
        with pytest.raises(ValueError, match=f"frame {frame} is incomplete"):
            y4m.read_header(str(q))
    q = tmp_path / "junk.y4m"
    q.write_bytes(whole[:34] + b"JUNK!" + whole[39:])
    with pytest.raises(ValueError, match="FRAME"):
        y4m.Y4MReader(str(q))


@pytest.mark.parametrize("chroma,H,W", [("420jpeg", 5, 7), ("420jpeg", 4, 16), ("444", 3, 5)])
def test_writer_reader_round_trip_on_the_cpu(tmp_path, chroma, H, W):
    frames = frames_of(7, H, W, 4, seed=5)
    path = str(tmp_path / "w.y4m")
    with y4m.Y4MWriter(path, W, H, fps=(30, 1), chroma=chroma, matrix="bt709", full_range=True, chunk=3) as w:
        w.write(frames[:5])
        w.write(frames[5:])
    assert w.frames_written == 7
    c = w.header.chroma
    planes = y4m.rgb8_to_yuv8(frames, c, "bt709", True)
    raw = open(path, "rb").read()
    head = f"YUV4MPEG2 W{W} H{H} F30:1 Ip A1:1 C{chroma} XCOLORRANGE=FULL\n".encode()
    assert raw == head + b"".join(b"FRAME\n" + b"".join(p[i].numpy().tobytes() for p in planes) for i in range(7))
    r = y4m.Y4MReader(path, chunk=2)
    assert len(r) == 7 and r.header.fps == (30, 1) and r.header.full_range
    want = y4m.yuv8_to_rgb8(*planes, c, "center", "bt709", True)
    assert torch.equal(r.frames("cpu", matrix="bt709"), want)
    assert torch.equal(r.frames("cpu", start=1, count=3, step=2, matrix="bt709"), want[1:7:2])
    assert torch.equal(r.frames("cpu", start=6, matrix="bt709"), want[6:])
    assert r.frames("cpu", start=7).shape == (0, H, W, 3)
    fl = y4m.load_clip(path, "cpu", start=2, count=2, layout="float", matrix="bt709")
    assert fl.dtype == torch.float32 and torch.equal(fl, want[2:4].permute(0, 3, 1, 2).to(torch.float32) / 255)
    for kw in (dict(start=8), dict(step=0), dict(start=2, count=6), dict(start=-1)):
        with pytest.raises(ValueError):
            r.frames("cpu", **kw)
    vids = y4m.videos_from_y4m(f"{path},{path}", "cpu", matrix="bt709")
    assert len(vids) == 2 and torch.equal(vids[1], want)


def test_writer_refusals(tmp_path):
    with pytest.raises(ValueError, match="chroma"):
        y4m.Y4MWriter(str(tmp_path / "x.y4m"), 4, 4, chroma="420mpeg2")
    with y4m.Y4MWriter(str(tmp_path / "x.y4m"), 4, 4, fps=29.97) as w:
        assert w.header.fps == (2997, 100)
        with pytest.raises(ValueError, match="frames are uint8"):
            w.write(torch.zeros(1, 4, 5, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="closed"):
        w.write(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))


# ---- the C side without a device ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from videoloop3d_amd import _lib
    return _lib


def test_abi_rows(L):
    assert C.sizeof(L.VideoDesc) == 72 and L.VideoDesc.y.offset == 40 and L.VideoDesc.frame_stride.offset == 64
    assert C.sizeof(L.VideoChoice) == 20
    for name in ("vl3d_video_coefs", "vl3d_video_choice", "vl3d_rgb8_to_yuv8", "vl3d_yuv8_to_rgb"):
        assert name in L.SIGNATURES and hasattr(L.lib(), name)


def test_the_library_holds_the_rules_integers(L):
    for matrix, full_range in COMBOS:
        enc, dec = (C.c_int32 * 12)(), (C.c_int32 * 10)()
        assert L.lib().vl3d_video_coefs(y4m.MATRIX_ID[matrix], int(full_range), enc, dec) == 0
        Cm, off = y4m.encode_coefs(matrix, full_range)
        D, y0 = y4m.decode_coefs(matrix, full_range)
        assert list(enc) == [v for row in Cm for v in row] + off
        assert list(dec) == [v for row in D for v in row] + [y0]
    assert L.lib().vl3d_video_coefs(2, 0, enc, dec) == 1


P = 4096      # a non-null, well aligned placeholder address: the choice function reads no memory


def desc_of(N=1, H=16, W=32, channels=3, chroma="420", siting="center", sink="u8", path=0, y=P, stride=None):
    return y4m._desc(N, H, W, channels, chroma, siting, "bt601", False, sink, y, y4m.frame_bytes(H, W, chroma) if stride is None else stride, path)


def choice(L, d, rgb=P, decode=False):
    out = L.VideoChoice()
    rc = L.lib().vl3d_video_choice(C.byref(d), C.c_void_p(rgb), int(decode), C.byref(out))
    return rc, out, (L.lib().vl3d_last_error() or b"").decode()


def test_choice_is_a_pure_function_of_the_call(L):
    rc, c, _ = choice(L, desc_of())
    assert rc == 0 and (c.wide, c.strip, c.rows, c.threads, c.blocks) == (1, 16, 2, 256, 1)
    rc, c, _ = choice(L, desc_of(chroma="444"), decode=True)
    assert rc == 0 and (c.wide, c.strip, c.rows) == (1, 16, 1)
    rc, c, _ = choice(L, desc_of(N=3, H=64, W=256))
    assert (c.wide, c.blocks) == (1, (3 * 32 * 16 + 255) // 256)
    byte_cases = [desc_of(W=24), desc_of(H=15), desc_of(W=33), desc_of(y=P + 1), desc_of(y=P + 8), desc_of(path=1),
                  desc_of(stride=y4m.frame_bytes(16, 32, "420") + 8)]
    for d in byte_cases:
        for decode in (False, True):
            rc, c, msg = choice(L, d, decode=decode)
            assert rc == 0 and c.wide == 0, msg
            assert (c.strip, c.rows) == ((1, 1) if decode else (2, 2))
    assert choice(L, desc_of(), rgb=P + 4)[1].wide == 0
    assert choice(L, desc_of(stride=y4m.frame_bytes(16, 32, "420") + 16))[1].wide == 1
    # a tight odd-sized I420 frame: U starts at an odd address
    d = desc_of(H=3, W=5)
    assert d.u % 2 == 1 and choice(L, d)[1].wide == 0


REFUSALS = [
    (dict(N=0), "N, H and W"), (dict(H=0), "N, H and W"), (dict(W=-1), "N, H and W"), (dict(channels=2), "channels"), (dict(channels=5), "channels"),
    (dict(chroma_id=2), "chroma"), (dict(siting_id=2), "siting_x"), (dict(matrix_id=2), "matrix"), (dict(range_id=2), "full_range"),
    (dict(sink_id=2), "sink"), (dict(path=2), "path"), (dict(stride=16 * 32), "frame_stride"), (dict(null="y"), "null plane"),
    (dict(null="u"), "null plane"), (dict(null="v"), "null plane"), (dict(null="rgb"), "null rgb"), (dict(N=3, H=32768, W=32768), "grid limit"),
]


def refused_call(L, entry, kw):
    kw = dict(kw)
    ids = {k: kw.pop(k) for k in ("chroma_id", "siting_id", "matrix_id", "range_id", "sink_id") if k in kw}
    null = kw.pop("null", None)
    d = desc_of(**kw)
    for k, v in ids.items():
        setattr(d, {"chroma_id": "chroma", "siting_id": "siting_x", "matrix_id": "matrix", "range_id": "full_range", "sink_id": "sink"}[k], v)
    if null in ("y", "u", "v"):
        setattr(d, null, None)
    rgb = None if null == "rgb" else C.c_void_p(P)
    if entry == "choice":
        rc = L.lib().vl3d_video_choice(C.byref(d), rgb, 0, C.byref(L.VideoChoice()))
    elif entry == "encode":
        rc = L.lib().vl3d_rgb8_to_yuv8(C.byref(d), rgb, None)
    else:
        rc = L.lib().vl3d_yuv8_to_rgb(C.byref(d), rgb, None)
    return rc, (L.lib().vl3d_last_error() or b"").decode()


@pytest.mark.parametrize("entry", ["choice", "encode", "decode"])
@pytest.mark.parametrize("kw,naming", REFUSALS)
def test_entries_refuse_before_any_launch(L, entry, kw, naming):
    """every refusal comes from the descriptor check, before anything touches a device: the placeholder addresses are never read"""
    rc, msg = refused_call(L, entry, kw)
    assert rc == 1 and naming in msg, (rc, msg)


def test_float_sink_refusals(L):
    d = desc_of(sink="float")
    assert L.lib().vl3d_yuv8_to_rgb(C.byref(d), C.c_void_p(P + 2), None) == 1 and b"4-byte aligned" in L.lib().vl3d_last_error()
    d = desc_of(sink="float", channels=4)
    assert L.lib().vl3d_yuv8_to_rgb(C.byref(d), C.c_void_p(P), None) == 1 and b"channels must be 3" in L.lib().vl3d_last_error()
    assert L.lib().vl3d_yuv8_to_rgb(None, C.c_void_p(P), None) == 1 and b"null descriptor" in L.lib().vl3d_last_error()


def test_device_wrappers_refuse_cpu_tensors(L):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        y4m.encode_frames(torch.zeros(1, 2, 2, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        y4m.decode_frames(torch.zeros(6, dtype=torch.uint8), 1, 2, 2)
