"""Video files without a codec: YUV4MPEG2 (.y4m) in and out, and the RGB <-> Y'CbCr rule both directions obey.

Three layers, top to bottom of this file:

  the rule     `rgb8_to_yuv8` / `yuv8_to_rgb8`: the conversion stated ONCE, in integers, in plain torch.  It runs wherever its tensors live and
               is the yardstick of every test, as baked.display_frames is for the display sink.  The kernels of csrc/vl3d_video.hip
               (vl3d_rgb8_to_yuv8 / vl3d_yuv8_to_rgb, docs/kernels/K10_video_io.md) store these bytes, byte for byte.
  the device   `encode_frames` / `decode_frames`: the two kernels on frames laid out as a .y4m payload holds them (planar Y, U, V per frame).
  the file     `Y4MHeader`, `read_header`, `Y4MReader`, `Y4MWriter`, `load_clip`, `videos_from_y4m`: pure host code around them.

A tensor on the CPU goes through the rule (the reader and the writer work without a device: the files are the same bytes); a tensor on the
device goes through the kernels.  Neither ever stands in for the other: a device tensor with no library is an error (_lib.lib()).

THE RULE.  Matrices BT.601 (Kr, Kb = 0.299, 0.114) and BT.709 (0.2126, 0.0722); limited range (Y' 16..235, C 16..240: scales 219/255,
224/255) or full; `matrix="auto"` is BT.709 for H >= 720, else BT.601 (what players assume of an untagged file).
  encode   the 3 x 3 float64 matrix with the range scale folded in, rounded to integers at 2^16; then the entry of largest magnitude of each
           row absorbs the rounding so that the chroma rows sum to exactly 0 (a grey has chroma 128) and the luma row to rint(sum 2^16)
           (white is white).  byte = clamp((sum_i c_i x_i + offset 2^16 + 2^15) >> 16, 0, 255), int32.  4:2:0 chroma: x_i are the SUMS over
           the 2 x 2 block (coordinates clamped at the right / bottom edge of an odd frame: always four samples, never a rounded mean) and
           the shift is 18.  Chroma planes ceil(H/2) x ceil(W/2), centre sited (C420jpeg).
  decode   chroma is upsampled bilinearly with clamped indices in exact integers, carried as 16 x chroma: centre siting has per-axis
           weights (1, 3) / 4 (chroma sample j sits at luma 2j + 0.5); siting_x = "left" (C420mpeg2) is co-sited with the even luma columns
           horizontally -- weights (1, 0) and (1/2, 1/2) -- and as above vertically.  The inverse matrix is in fixed point at 2^21 (the
           chroma columns at 2^17, for the 16 x): the largest scale at which every intermediate fits int32 (decode_extremes()).
           byte = clamp((cy (Y - y0) + cu (U16 - 2048) + cv (V16 - 2048) + 2^20) >> 21, 0, 255).  Sinks: uint8 [N,H,W,3] and
           float32 [N,3,H,W] = byte / 255.
"""
import os
from collections import namedtuple

import numpy as np
import torch

MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
MATRIX_ID = {"bt601": 0, "bt709": 1}
CHROMA_ID = {"444": 0, "420": 1}
SITING_ID = {"center": 0, "left": 1}
SINK_ID = {"u8": 0, "float": 1}
ENC_SHIFT = 16
DEC_SHIFT = 21      # luma column; the chroma columns multiply 16 x chroma and sit at DEC_SHIFT - 4
PATH_AUTO, PATH_BYTE = 0, 1
PATHS = {0: "byte", 1: "wide"}


def resolve_matrix(matrix, H):
    """'auto' -> 'bt709' for H >= 720 else 'bt601'; a name of MATRICES passes; a (Kr, Kb) pair passes (tests plant faults with it)."""
    if isinstance(matrix, tuple):
        return matrix
    if matrix == "auto":
        return "bt709" if H >= 720 else "bt601"
    if matrix not in MATRICES:
        raise ValueError(f"matrix must be 'auto', 'bt601' or 'bt709', got {matrix!r}")
    return matrix


def _kr_kb(matrix):
    return matrix if isinstance(matrix, tuple) else MATRICES[matrix]


def forward_matrix(matrix, full_range):
    """float64 (M [3,3], offset [3]): Y'CbCr bytes = M rgb + offset before rounding (range scale folded in)."""
    Kr, Kb = _kr_kb(matrix)
    Kg = 1 - Kr - Kb
    sy = 1.0 if full_range else 219 / 255
    sc = 1.0 if full_range else 224 / 255
    M = np.array([[Kr, Kg, Kb],
                  [-Kr / (2 * (1 - Kb)), -Kg / (2 * (1 - Kb)), 0.5],
                  [0.5, -Kg / (2 * (1 - Kr)), -Kb / (2 * (1 - Kr))]], dtype=np.float64)
    M[0] *= sy
    M[1:] *= sc
    return M, np.array([0.0 if full_range else 16.0, 128.0, 128.0])


def inverse_matrix(matrix, full_range):
    """float64 (A [3,3], y0): rgb = A (Y - y0, Cb - 128, Cr - 128) before rounding."""
    Kr, Kb = _kr_kb(matrix)
    Kg = 1 - Kr - Kb
    sy = 1.0 if full_range else 219 / 255
    sc = 1.0 if full_range else 224 / 255
    A = np.array([[1 / sy, 0.0, 2 * (1 - Kr) / sc],
                  [1 / sy, -2 * Kb * (1 - Kb) / Kg / sc, -2 * Kr * (1 - Kr) / Kg / sc],
                  [1 / sy, 2 * (1 - Kb) / sc, 0.0]], dtype=np.float64)
    return A, (0 if full_range else 16)


def encode_coefs(matrix, full_range):
    """the integers of the encode rule: (C [3][3] at 2^16 with the row sums repaired, offsets [3])."""
    M, off = forward_matrix(matrix, full_range)
    C = np.rint(M * (1 << ENC_SHIFT)).astype(np.int64)
    want = [int(np.rint(M[0].sum() * (1 << ENC_SHIFT))), 0, 0]
    for i in range(3):
        j = int(np.argmax(np.abs(C[i])))
        C[i, j] += want[i] - int(C[i].sum())
    return [[int(v) for v in row] for row in C], [int(v) for v in off]


def decode_coefs(matrix, full_range):
    """the integers of the decode rule: (D [3][3]: per output channel (cy at 2^21, cu, cv at 2^17), y0)."""
    A, y0 = inverse_matrix(matrix, full_range)
    D = [[int(np.rint(A[c, 0] * (1 << DEC_SHIFT))), int(np.rint(A[c, 1] * (1 << (DEC_SHIFT - 4)))), int(np.rint(A[c, 2] * (1 << (DEC_SHIFT - 4))))]
         for c in range(3)]
    return D, y0


def decode_extremes(matrix, full_range):
    """(lowest, highest) value the decode accumulator -- rounding term included -- takes over all byte inputs, as Python integers: every
    term is linear in its input, so the extremes sit at the ends of each input's range."""
    D, y0 = decode_coefs(matrix, full_range)
    lo = hi = None
    for cy, cu, cv in D:
        terms = [(cy * (0 - y0), cy * (255 - y0)), (cu * (0 - 2048), cu * (16 * 255 - 2048)), (cv * (0 - 2048), cv * (16 * 255 - 2048))]
        a = sum(min(t) for t in terms) + (1 << (DEC_SHIFT - 1))
        b = sum(max(t) for t in terms) + (1 << (DEC_SHIFT - 1))
        lo, hi = (a if lo is None else min(lo, a)), (b if hi is None else max(hi, b))
    return lo, hi


def chroma_size(H, W, chroma):
    return ((H + 1) // 2, (W + 1) // 2) if chroma == "420" else (H, W)


def frame_bytes(H, W, chroma):
    ch, cw = chroma_size(H, W, chroma)
    return H * W + 2 * ch * cw


def _check_chroma(chroma):
    if chroma not in CHROMA_ID:
        raise ValueError(f"chroma must be '444' or '420', got {chroma!r}")


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
def rgb8_to_yuv8(frames, chroma="420", matrix="auto", full_range=False):
    """THE encode rule: frames uint8 [N,H,W,3|4] (a fourth channel is not read) -> (y [N,H,W], u, v [N,ch,cw]) uint8."""
    _check_chroma(chroma)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] not in (3, 4):
        raise ValueError(f"rgb8_to_yuv8: frames are uint8 [N,H,W,3|4], got {frames.dtype} {tuple(frames.shape)}")
    N, H, W, _ = frames.shape
    C, off = encode_coefs(resolve_matrix(matrix, H), full_range)
    x = frames[..., :3].to(torch.int32)

    def row(i, v, shift):
        acc = C[i][0] * v[..., 0] + C[i][1] * v[..., 1] + C[i][2] * v[..., 2] + ((off[i] << shift) + (1 << (shift - 1)))
        return (acc >> shift).clamp(0, 255).to(torch.uint8)

    y = row(0, x, ENC_SHIFT)
    if chroma == "444":
        return y, row(1, x, ENC_SHIFT), row(2, x, ENC_SHIFT)
    ch, cw = chroma_size(H, W, chroma)
    r0 = torch.arange(ch, device=frames.device) * 2
    c0 = torch.arange(cw, device=frames.device) * 2
    r1, c1 = (r0 + 1).clamp(max=H - 1), (c0 + 1).clamp(max=W - 1)
    s = x[:, r0][:, :, c0] + x[:, r0][:, :, c1] + x[:, r1][:, :, c0] + x[:, r1][:, :, c1]
    return y, row(1, s, ENC_SHIFT + 2), row(2, s, ENC_SHIFT + 2)


def upsample_chroma16(c, H, W, chroma="420", siting_x="center"):
    """chroma plane uint8 [N,ch,cw] -> int32 [N,H,W] = 16 x the bilinear upsample, clamped indices, exact."""
    c = c.to(torch.int32)
    if chroma == "444":
        return c * 16
    ch, cw = c.shape[-2:]
    dev = c.device
    yy, xx = torch.arange(H, device=dev), torch.arange(W, device=dev)
    # per axis: luma k reads chroma (k >> 1) with weight 3 and its neighbour on the side of k's parity ((k >> 1) - 1 | + 1) with weight 1
    ja = (yy >> 1).clamp(max=ch - 1)
    jb = ((yy >> 1) + (yy & 1) * 2 - 1).clamp(0, ch - 1)
    v = 3 * c[:, ja] + c[:, jb]                               # [N,H,cw], x 4
    if siting_x == "center":
        ia = (xx >> 1).clamp(max=cw - 1)
        ib = ((xx >> 1) + (xx & 1) * 2 - 1).clamp(0, cw - 1)
        return 3 * v[:, :, ia] + v[:, :, ib]
    if siting_x != "left":
        raise ValueError(f"siting_x must be 'center' or 'left', got {siting_x!r}")
    ia = (xx >> 1).clamp(max=cw - 1)
    ib = ((xx >> 1) + (xx & 1)).clamp(max=cw - 1)              # even: itself again (weights (1, 0)); odd: the right neighbour (1/2, 1/2)
    return 2 * v[:, :, ia] + 2 * v[:, :, ib]


def yuv8_to_rgb8(y, u, v, chroma="420", siting_x="center", matrix="auto", full_range=False, layout="u8"):
    """THE decode rule: y uint8 [N,H,W], u, v uint8 [N,ch,cw] -> uint8 [N,H,W,3] (layout 'u8') or float32 [N,3,H,W] = byte / 255 ('float')."""
    _check_chroma(chroma)
    if layout not in SINK_ID:
        raise ValueError(f"layout must be 'u8' or 'float', got {layout!r}")
    N, H, W = y.shape
    if tuple(u.shape) != (N,) + chroma_size(H, W, chroma) or u.shape != v.shape:
        raise ValueError(f"yuv8_to_rgb8: chroma planes of {tuple(u.shape)} / {tuple(v.shape)} for luma {tuple(y.shape)}, chroma {chroma}")
    D, y0 = decode_coefs(resolve_matrix(matrix, H), full_range)
    yl = y.to(torch.int32) - y0
    ul = upsample_chroma16(u, H, W, chroma, siting_x) - 2048
    vl = upsample_chroma16(v, H, W, chroma, siting_x) - 2048
    out = [((cy * yl + cu * ul + cv * vl + (1 << (DEC_SHIFT - 1))) >> DEC_SHIFT).clamp(0, 255).to(torch.uint8) for cy, cu, cv in D]
    if layout == "u8":
        return torch.stack(out, dim=-1)
    return torch.stack(out, dim=1).to(torch.float32) / 255


# ---- the device: frames as a .y4m payload holds them -------------------------------------------------------------------------------------
def _desc(N, H, W, channels, chroma, siting_x, matrix, full_range, sink, y_ptr, stride, path):
    from . import _lib
    ch, cw = chroma_size(H, W, chroma)
    d = _lib.VideoDesc()
    d.N, d.H, d.W, d.channels = N, H, W, channels
    d.chroma, d.siting_x, d.matrix, d.full_range = CHROMA_ID[chroma], SITING_ID[siting_x], MATRIX_ID[resolve_matrix(matrix, H)], int(bool(full_range))
    d.sink, d.path = SINK_ID[sink], int(path)
    d.y, d.u, d.v = y_ptr, y_ptr + H * W, y_ptr + H * W + ch * cw
    d.frame_stride = int(stride)
    return d


def video_choice(d, rgb_ptr, decode):
    """which path a call takes ('wide' | 'byte'), from the library's own pure function (vl3d_video_choice): nothing is launched."""
    from . import _lib
    import ctypes as C
    out = _lib.VideoChoice()
    _lib.check(_lib.lib().vl3d_video_choice(C.byref(d), C.c_void_p(rgb_ptr), int(bool(decode)), C.byref(out)), "vl3d_video_choice")
    return PATHS[out.wide]


def planes_of(buf, N, H, W, chroma, stride=None):
    """views (y [N,H,W], u, v [N,ch,cw]) of a uint8 buffer holding N frames `stride` bytes apart, each planar Y, U, V and tight."""
    ch, cw = chroma_size(H, W, chroma)
    fb = frame_bytes(H, W, chroma)
    stride = fb if stride is None else stride
    flat = buf.reshape(-1)
    return (flat.as_strided((N, H, W), (stride, W, 1), 0), flat.as_strided((N, ch, cw), (stride, cw, 1), H * W),
            flat.as_strided((N, ch, cw), (stride, cw, 1), H * W + ch * cw))


def _payload(buf, N, H, W, chroma, stride, what):
    fb = frame_bytes(H, W, chroma)
    stride = fb if stride is None else int(stride)
    if buf.dtype != torch.uint8 or buf.dim() != 1 or not buf.is_contiguous() or stride < fb or buf.numel() < (N - 1) * stride + fb:
        raise ValueError(f"{what}: the payload is a contiguous 1-D uint8 tensor of at least (N - 1) * stride + {fb} bytes with stride >= {fb}")
    return stride


def encode_frames(frames, buf=None, stride=None, chroma="420", matrix="auto", full_range=False, path=PATH_AUTO):
    """vl3d_rgb8_to_yuv8: device frames uint8 [N,H,W,3|4] -> `buf` (1-D uint8; allocated when None), N frames `stride` bytes apart
    (default: tight), each planar Y, U, V -- the rule's bytes, on the current stream.  Returns buf; planes_of() views it."""
    from . import _lib
    import ctypes as C
    _check_chroma(chroma)
    _lib.check_cuda(frames, buf)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or not frames.is_contiguous():
        raise ValueError(f"encode_frames: frames are contiguous uint8 [N,H,W,3|4], got {frames.dtype} {tuple(frames.shape)}")
    N, H, W, channels = frames.shape
    if buf is None:
        stride = frame_bytes(H, W, chroma) if stride is None else stride
        buf = torch.empty(N * stride, dtype=torch.uint8, device=frames.device)
    stride = _payload(buf, N, H, W, chroma, stride, "encode_frames")
    d = _desc(N, H, W, channels, chroma, "center", matrix, full_range, "u8", buf.data_ptr(), stride, path)
    _lib.check(_lib.lib().vl3d_rgb8_to_yuv8(C.byref(d), _lib.ptr(frames), _lib.stream_ptr(frames.device)), "vl3d_rgb8_to_yuv8")
    return buf


def decode_frames(buf, N, H, W, stride=None, chroma="420", siting_x="center", matrix="auto", full_range=False, layout="u8", channels=3,
                  out=None, path=PATH_AUTO):
    """vl3d_yuv8_to_rgb: `buf` as encode_frames fills it -> uint8 [N,H,W,channels] (layout 'u8'; a fourth channel is 255) or float32
    [N,3,H,W] ('float'), the rule's bytes, on the current stream.  `out`: written in place."""
    from . import _lib
    import ctypes as C
    _check_chroma(chroma)
    _lib.check_cuda(buf, out)
    stride = _payload(buf, N, H, W, chroma, stride, "decode_frames")
    if layout not in SINK_ID:
        raise ValueError(f"layout must be 'u8' or 'float', got {layout!r}")
    shape, dtype = ((N, H, W, channels), torch.uint8) if layout == "u8" else ((N, 3, H, W), torch.float32)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=buf.device)
    elif tuple(out.shape) != shape or out.dtype != dtype or not out.is_contiguous():
        raise ValueError(f"decode_frames: `out` must be contiguous {dtype} {shape}")
    d = _desc(N, H, W, channels if layout == "u8" else 3, chroma, siting_x, matrix, full_range, layout, buf.data_ptr(), stride, path)
    _lib.check(_lib.lib().vl3d_yuv8_to_rgb(C.byref(d), _lib.ptr(out), _lib.stream_ptr(buf.device)), "vl3d_yuv8_to_rgb")
    return out


# ---- the file ---------------------------------------------------------------------------------------------------------------------------
MAGIC = b"YUV4MPEG2"
_CTAGS = {"420jpeg": ("420", "center"), "420mpeg2": ("420", "left"), "420": ("420", "center"), "444": ("444", "center")}
_REFUSED_C = {"420paldv": "C420paldv (PAL-DV chroma siting) is not read", "422": "C422 (4:2:2) is not read", "411": "C411 (4:1:1) is not read",
              "mono": "Cmono (no chroma planes) is not read"}

Y4MHeader = namedtuple("Y4MHeader", "W H fps interlace aspect ctag colorrange")
Y4MHeader.__doc__ = """The stream header of a .y4m file: W, H; fps = (n, d) of `Fn:d`; interlace 'p' or None (no I tag); aspect = (n, d) of `An:d` or None;
ctag: the C tag without its letter ('420jpeg', '420mpeg2', '420', '444') or None (no C tag: 4:2:0, centre sited); colorrange 'FULL',
'LIMITED' or None (no XCOLORRANGE).  .chroma / .siting_x / .full_range give what the conversion takes."""
Y4MHeader.chroma = property(lambda h: _CTAGS[h.ctag or "420"][0])
Y4MHeader.siting_x = property(lambda h: _CTAGS[h.ctag or "420"][1])
Y4MHeader.full_range = property(lambda h: h.colorrange == "FULL")
Y4MHeader.frame_bytes = property(lambda h: frame_bytes(h.H, h.W, h.chroma))


def _ratio(tag, text):
    try:
        n, d = text.split(":")
        n, d = int(n), int(d)
    except ValueError:
        raise ValueError(f"y4m: tag {tag}{text} is not a ratio n:d") from None
    return n, d


def parse_header(line):
    """the stream header line (bytes, without its newline) -> Y4MHeader; every refusal names the tag."""
    parts = line.split(b" ")
    if parts[0] != MAGIC:
        raise ValueError(f"y4m: the file does not start with the magic {MAGIC.decode()} (got {line[:16]!r})")
    W = H = None
    fps, interlace, aspect, ctag, colorrange = (25, 1), None, None, None, None
    for p in parts[1:]:
        if not p:
            continue
        tag, text = chr(p[0]), p[1:].decode("ascii", "replace")
        if tag == "W":
            W = int(text)
        elif tag == "H":
            H = int(text)
        elif tag == "F":
            fps = _ratio("F", text)
        elif tag == "A":
            aspect = _ratio("A", text)
        elif tag == "I":
            if text != "p":
                raise ValueError(f"y4m: tag I{text}: interlaced streams (It, Ib, Im) are not read, progressive Ip only")
            interlace = "p"
        elif tag == "C":
            if any(text.endswith(d) for d in ("p10", "p12", "p14", "p16")):
                raise ValueError(f"y4m: tag C{text}: 8-bit samples only, high bit depths (p10 / p12 / p16) are not read")
            if text in _REFUSED_C:
                raise ValueError(f"y4m: tag C{text}: {_REFUSED_C[text]}")
            if text not in _CTAGS:
                raise ValueError(f"y4m: tag C{text}: unknown chroma format (read are C420jpeg, C420mpeg2, C420, C444)")
            ctag = text
        elif tag == "X":
            if text.startswith("COLORRANGE="):
                colorrange = text[len("COLORRANGE="):]
                if colorrange not in ("FULL", "LIMITED"):
                    raise ValueError(f"y4m: tag X{text}: XCOLORRANGE is FULL or LIMITED")
    if W is None or W < 1:
        raise ValueError("y4m: the header has no W tag (frame width)")
    if H is None or H < 1:
        raise ValueError("y4m: the header has no H tag (frame height)")
    return Y4MHeader(W, H, fps, interlace, aspect, ctag, colorrange)


def format_header(h):
    tags = [MAGIC.decode(), f"W{h.W}", f"H{h.H}", f"F{h.fps[0]}:{h.fps[1]}"]
    if h.interlace:
        tags.append(f"I{h.interlace}")
    if h.aspect:
        tags.append(f"A{h.aspect[0]}:{h.aspect[1]}")
    if h.ctag:
        tags.append(f"C{h.ctag}")
    if h.colorrange:
        tags.append(f"XCOLORRANGE={h.colorrange}")
    return (" ".join(tags) + "\n").encode("ascii")


def _index(path):
    """-> (Y4MHeader, [payload offset of every frame]).  FRAME lines may carry parameters, so they are walked, not computed; the file must be
    header + whole frames."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(4096)
        end = head.find(b"\n")
        if not head.startswith(MAGIC) or end < 0:
            raise ValueError(f"y4m: {path} does not start with a {MAGIC.decode()} header line (magic missing)")
        h = parse_header(head[:end])
        fb, pos, offsets = h.frame_bytes, end + 1, []
        while pos < size:
            f.seek(pos)
            line = f.read(256)
            nl = line.find(b"\n")
            if not line.startswith(b"FRAME") or nl < 0 or (nl > 5 and line[5:6] != b" "):
                if b"FRAME\n".startswith(line) or (line.startswith(b"FRAME") and nl < 0 and len(line) < 256):
                    raise ValueError(f"y4m: {path} is not header + whole frames: frame {len(offsets)} is incomplete (its FRAME line is cut)")
                raise ValueError(f"y4m: {path}: no FRAME line where frame {len(offsets)} should start (offset {pos})")
            if pos + nl + 1 + fb > size:
                raise ValueError(f"y4m: {path} is not header + whole frames: frame {len(offsets)} is incomplete "
                                 f"({size - pos - nl - 1} of {fb} payload bytes)")
            offsets.append(pos + nl + 1)
            pos += nl + 1 + fb
    return h, offsets


def read_header(path):
    """The stream header of a .y4m file, after checking that the file is header + whole frames."""
    return _index(path)[0]


def _align(n, a=256):
    return (n + a - 1) // a * a


class Y4MReader:
    """A .y4m file as frames.  len(): its frames; .header: Y4MHeader.  `chunk`: frames per transfer."""

    def __init__(self, path, chunk=16):
        self.path, self.chunk = str(path), max(1, int(chunk))
        self.header, self._offsets = _index(self.path)

    def __len__(self):
        return len(self._offsets)

    def _selection(self, start, count, step):
        n = len(self)
        if step < 1 or start < 0 or start > n:
            raise ValueError(f"Y4MReader: start {start}, step {step} for a file of {n} frames (start in 0..{n}, step >= 1)")
        idx = list(range(start, n, step))
        if count is not None:
            if count < 0 or count > len(idx):
                raise ValueError(f"Y4MReader: count {count} from frame {start} in steps of {step}: the file has {len(idx)} such frames")
            idx = idx[:count]
        return idx

    def frames(self, device, start=0, count=None, step=1, layout="u8", matrix="auto"):
        """frames start, start + step, ... (`count` of them; None: to the end) -> uint8 [n,H,W,3] ('u8') or float32 [n,3,H,W] = byte / 255
        ('float') on `device`.  On the device: every frame's payload is read into an aligned slot of one of two pinned buffers, a chunk at
        a time; the chunk goes up on a side stream and is decoded on the current one (vl3d_yuv8_to_rgb) while the host reads the next."""
        h, dev = self.header, torch.device(device)
        idx = self._selection(start, count, step)
        if layout not in SINK_ID:
            raise ValueError(f"layout must be 'u8' or 'float', got {layout!r}")
        n, fb = len(idx), h.frame_bytes
        kw = dict(chroma=h.chroma, siting_x=h.siting_x, matrix=matrix, full_range=h.full_range, layout=layout)
        shape, dtype = ((n, h.H, h.W, 3), torch.uint8) if layout == "u8" else ((n, 3, h.H, h.W), torch.float32)
        out = torch.empty(shape, dtype=dtype, device=dev)
        if n == 0:
            return out
        slot = _align(fb)
        chunk = min(self.chunk, n)
        on_dev = dev.type == "cuda"
        host = [torch.empty(chunk * slot, dtype=torch.uint8, pin_memory=on_dev) for _ in range(2 if on_dev else 1)]
        if on_dev:
            cur, side = torch.cuda.current_stream(dev), torch.cuda.Stream(dev)
            staged = [torch.empty(chunk * slot, dtype=torch.uint8, device=dev) for _ in range(2)]
            up, done = [torch.cuda.Event() for _ in range(2)], [None, None]
        with open(self.path, "rb", buffering=0) as f:
            for k, c0 in enumerate(range(0, n, chunk)):
                m, b = min(chunk, n - c0), (k % 2 if on_dev else 0)
                if on_dev and done[b] is not None:
                    done[b].synchronize()      # the chunk that last used this pair of buffers is decoded: both are free
                view = host[b].numpy()
                for i in range(m):
                    f.seek(self._offsets[idx[c0 + i]])
                    if f.readinto(memoryview(view[i * slot:i * slot + fb])) != fb:
                        raise IOError(f"y4m: {self.path}: short read in frame {idx[c0 + i]}")
                if not on_dev:
                    y, u, v = planes_of(host[0], m, h.H, h.W, h.chroma, slot)
                    out[c0:c0 + m] = yuv8_to_rgb8(y, u, v, **kw)
                    continue
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    staged[b][:m * slot].copy_(host[b][:m * slot], non_blocking=True)
                    up[b].record(side)
                cur.wait_event(up[b])
                decode_frames(staged[b], m, h.H, h.W, stride=slot, out=out[c0:c0 + m], **kw)
                done[b] = torch.cuda.Event()
                done[b].record(cur)
        if on_dev:
            for e in done:
                if e is not None:
                    e.synchronize()      # the pinned and staging buffers are released below: nothing may still read them
        return out


def load_clip(path, device, start=0, count=None, step=1, layout="u8", matrix="auto", chunk=16):
    """One call: the frames of a .y4m file on `device` (Y4MReader.frames)."""
    return Y4MReader(path, chunk=chunk).frames(device, start=start, count=count, step=step, layout=layout, matrix=matrix)


def videos_from_y4m(paths, device, layout="u8", **kw):
    """[path, ...] -> the list of clips train_3dvid.train / evaluations.evaluate_views take: uint8 [F,H,W,3] per view (layout 'float':
    float32 [F,3,H,W] in 0..1, what MVVidPatchDataset takes), on `device`."""
    if isinstance(paths, (str, os.PathLike)):
        paths = [p for p in str(paths).split(",") if p]
    return [load_clip(p, device, layout=layout, **kw) for p in paths]


class Y4MWriter:
    """Frames to a .y4m file.  A context manager; write(frames) takes uint8 [n,H,W,3|4] (on the device: converted by vl3d_rgb8_to_yuv8 on the
    caller's stream into staging this writer owns, copied to one of two pinned buffers, and written to the file once that buffer's event
    has fired -- at a later write() or at close(); write() itself waits for no file and no device, and `frames` may be overwritten on the
    same stream as soon as it returns).  `chunk`: frames per buffer."""

    def __init__(self, path, W, H, fps=(25, 1), chroma="420jpeg", matrix="auto", full_range=False, chunk=16):
        if chroma not in ("420jpeg", "444"):
            raise ValueError(f"Y4MWriter: chroma is '420jpeg' or '444' (a box average is centre sited), got {chroma!r}")
        if isinstance(fps, (int, float)):
            from fractions import Fraction
            fr = Fraction(fps).limit_denominator(1001)
            fps = (fr.numerator, fr.denominator)
        self.header = Y4MHeader(int(W), int(H), (int(fps[0]), int(fps[1])), "p", (1, 1), chroma, "FULL" if full_range else "LIMITED")
        self.matrix, self.chunk = resolve_matrix(matrix, int(H)), max(1, int(chunk))
        self.path, self.frames_written = str(path), 0
        self._f = open(self.path, "wb")
        self._f.write(format_header(self.header))
        self._slot = _align(self.header.frame_bytes)
        self._k, self._host, self._staged, self._pending = 0, [None, None], [None, None], [None, None]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _to_file(self, view, m):
        fb, slot = self.header.frame_bytes, self._slot
        for i in range(m):
            self._f.write(b"FRAME\n")
            self._f.write(memoryview(view[i * slot:i * slot + fb]))
        self.frames_written += m

    def _drain(self, b):
        if self._pending[b] is not None:
            ev, m = self._pending[b]
            ev.synchronize()
            self._to_file(self._host[b].numpy(), m)
            self._pending[b] = None

    def write(self, frames):
        h = self.header
        if frames.dtype != torch.uint8 or frames.dim() != 4 or tuple(frames.shape[1:3]) != (h.H, h.W) or frames.shape[3] not in (3, 4):
            raise ValueError(f"Y4MWriter.write: frames are uint8 [n,{h.H},{h.W},3|4], got {frames.dtype} {tuple(frames.shape)}")
        if self._f is None:
            raise ValueError("Y4MWriter.write: the writer is closed")
        kw = dict(chroma=h.chroma, matrix=self.matrix, full_range=h.full_range)
        slot, fb = self._slot, h.frame_bytes
        for c0 in range(0, len(frames), self.chunk):
            part = frames[c0:c0 + self.chunk]
            m = len(part)
            if not frames.is_cuda:
                y, u, v = rgb8_to_yuv8(part, **kw)
                buf = torch.empty(m * slot, dtype=torch.uint8)
                for dst, src in zip(planes_of(buf, m, h.H, h.W, h.chroma, slot), (y, u, v)):
                    dst.copy_(src)
                self._to_file(buf.numpy(), m)
                continue
            b = self._k % 2
            self._k += 1
            self._drain(b)      # this pair of buffers is free once its bytes are with the file
            if self._host[b] is None:
                self._host[b] = torch.empty(self.chunk * slot, dtype=torch.uint8, pin_memory=True)
                self._staged[b] = torch.empty(self.chunk * slot, dtype=torch.uint8, device=frames.device)
            encode_frames(part.contiguous(), self._staged[b], stride=slot, **kw)
            self._host[b][:m * slot].copy_(self._staged[b][:m * slot], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(frames.device))
            self._pending[b] = (ev, m)

    def close(self):
        if self._f is None:
            return
        for b in (self._k % 2, (self._k + 1) % 2):      # the older buffer first: frames reach the file in order
            self._drain(b)
        self._f.close()
        self._f = None
