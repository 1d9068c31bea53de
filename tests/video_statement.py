"""The statement the video conversion is held to: the float64 DEFINITION of RGB <-> Y'CbCr (the ITU matrices, the range scale,
floor(x + 0.5), the bilinear chroma upsample in float64) and the comparison of bytes against it.

Nothing here is taken from videoloop3d_amd.y4m but the rule's own INTEGER coefficients, and those only to size the band around the .5 ties
inside which a fixed-point rule may round the other way:  delta = sum_i |c_i / 2^s - m_i| * (largest |input_i|)  is the furthest the rule's
exact-arithmetic value can lie from the definition's, so
  * a byte equals the definition's rounding wherever the definition's value is further than delta from a tie,
  * inside the band it differs by at most 1,
  * and at most 2 % of the compared values may lie inside the band (a condition on the rule: a coarser scale would widen the band until
    the first statement says nothing).
`compare` asserts the three and prints the share in the band.  The share is a statement about a population: frames of a handful of pixels
are pooled (`compare_pooled`) with the other sizes of their case before it is taken -- one value of eighteen in the band is 5.6 %.
"""
import numpy as np

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
BAND_CAP = 0.02


def definition_forward(matrix, full_range):
    """float64 (M, offset): Y'CbCr = M rgb + offset.  BT.601 / BT.709 luma weights; Cb = (B - Y) / (2 (1 - Kb)), Cr = (R - Y) / (2 (1 - Kr));
    limited range scales luma by 219 / 255 (+16) and chroma by 224 / 255; chroma sits at 128."""
    Kr, Kb = KR_KB[matrix] if isinstance(matrix, str) else matrix
    Kg = 1.0 - Kr - Kb
    Y = np.array([Kr, Kg, Kb])
    Cb = (np.array([0.0, 0.0, 1.0]) - Y) / (2 * (1 - Kb))
    Cr = (np.array([1.0, 0.0, 0.0]) - Y) / (2 * (1 - Kr))
    sy, sc = (1.0, 1.0) if full_range else (219 / 255, 224 / 255)
    return np.stack([Y * sy, Cb * sc, Cr * sc]), np.array([0.0 if full_range else 16.0, 128.0, 128.0])


def definition_inverse(matrix, full_range):
    """float64 (A, y0): rgb = A (Y' - y0, Cb - 128, Cr - 128): the inverse of definition_forward, by numpy."""
    M, off = definition_forward(matrix, full_range)
    return np.linalg.inv(M), off[0]


def encode_values(rgb, chroma, matrix, full_range):
    """the definition's UNROUNDED planes: rgb [N,H,W,3] (any integer dtype) -> (y [N,H,W], u, v [N,ch,cw]) float64.  4:2:0 chroma is the
    matrix applied to the MEAN of the 2 x 2 block, coordinates clamped at the right / bottom edge (centre siting)."""
    M, off = definition_forward(matrix, full_range)
    x = np.asarray(rgb)[..., :3].astype(np.float64)
    y = x @ M[0] + off[0]
    if chroma == "420":
        H, W = x.shape[1:3]
        r0, c0 = np.arange(0, H, 2), np.arange(0, W, 2)
        r1, c1 = np.minimum(r0 + 1, H - 1), np.minimum(c0 + 1, W - 1)
        x = (x[:, r0][:, :, c0] + x[:, r0][:, :, c1] + x[:, r1][:, :, c0] + x[:, r1][:, :, c1]) / 4
    return y, x @ M[1] + off[1], x @ M[2] + off[2]


def upsample_values(c, H, W, chroma, siting_x):
    """the definition's chroma at every luma position, float64 [N,H,W]: bilinear between the chroma samples, sample j at luma 2 j + 0.5
    (centre) or at luma 2 j (left, horizontally only), positions outside the outermost samples take the outermost sample."""
    c = np.asarray(c).astype(np.float64)
    if chroma == "444":
        return c

    def axis(v, n, ax, shift):
        pos = (np.arange(n) - shift) / 2.0                      # luma k in chroma coordinates
        i0 = np.floor(pos).astype(np.int64)
        w1 = pos - i0
        m = v.shape[ax]
        a, b = np.clip(i0, 0, m - 1), np.clip(i0 + 1, 0, m - 1)
        shape = [1] * v.ndim
        shape[ax] = n
        return np.take(v, a, axis=ax) * (1 - w1).reshape(shape) + np.take(v, b, axis=ax) * w1.reshape(shape)

    return axis(axis(c, H, 1, 0.5), W, 2, 0.5 if siting_x == "center" else 0.0)


def decode_values(y, u, v, chroma, siting_x, matrix, full_range):
    """the definition's UNROUNDED rgb, float64 [N,H,W,3]."""
    A, y0 = definition_inverse(matrix, full_range)
    N, H, W = np.asarray(y).shape
    t = np.stack([np.asarray(y).astype(np.float64) - y0, upsample_values(u, H, W, chroma, siting_x) - 128.0,
                  upsample_values(v, H, W, chroma, siting_x) - 128.0], axis=-1)
    return t @ A.T


def round_bytes(x):
    return np.clip(np.floor(x + 0.5), 0, 255).astype(np.int64)


def encode_delta(C, matrix, full_range):
    """band half-width per output row (Y, U, V) from the rule's integer rows C [3][3] at 2^16: every input is at most 255."""
    M, _ = definition_forward(matrix, full_range)
    return np.abs(np.asarray(C, dtype=np.float64) / 65536.0 - M).sum(axis=1) * 255.0


def decode_delta(D, matrix, full_range):
    """band half-width per output channel from the rule's integers D [3][3] (cy at 2^21; cu, cv at 2^17 on 16 x chroma, i.e. at 2^21 on
    chroma): |Y' - y0| <= 255, |C - 128| <= 128."""
    A, _ = definition_inverse(matrix, full_range)
    D = np.asarray(D, dtype=np.float64) / float(1 << 21)
    D[:, 1:] *= 16.0
    return (np.abs(D - A) * np.array([255.0, 128.0, 128.0])).sum(axis=1)


def compare(got, value, delta, what, cap=BAND_CAP):
    """got: bytes of the code under test; value: the definition's unrounded float64 values, same shape; delta: the band's half-width.
    Asserts the three statements of this module; returns (share in the band, number of bytes that differ)."""
    got = np.asarray(got).astype(np.int64)
    value = np.asarray(value, dtype=np.float64)
    assert got.shape == value.shape, f"{what}: shapes {got.shape} / {value.shape}"
    want = round_bytes(value)
    frac = value + 0.5 - np.floor(value + 0.5)
    band = np.minimum(frac, 1.0 - frac) < delta
    diff = np.abs(got - want)
    share = float(band.mean()) if band.size else 0.0
    print(f"{what}: {got.size} values, delta {float(np.max(delta)):.5f} LSB, {100 * share:.3f} % in the band, {int((diff > 0).sum())} differ")
    outside = int(((diff > 0) & ~band).sum())
    assert outside == 0, f"{what}: {outside} bytes differ from the float64 rounding outside the tie band (largest difference {int(diff.max())})"
    assert int(diff.max(initial=0)) <= 1, f"{what}: a byte differs by {int(diff.max())} inside the band"
    assert share <= cap, f"{what}: {100 * share:.2f} % of the values lie in the tie band (cap {100 * cap:.0f} %)"
    return share, int((diff > 0).sum())


def compare_pooled(items, what, cap=BAND_CAP):
    """items: [(got, value, delta)] of any shapes (delta broadcast against value) -> compare() over all of them as one population."""
    got = np.concatenate([np.asarray(g).astype(np.int64).reshape(-1) for g, _, _ in items])
    value = np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1) for _, v, _ in items])
    delta = np.concatenate([np.broadcast_to(np.asarray(d, dtype=np.float64), np.asarray(v).shape).reshape(-1) for _, v, d in items])
    return compare(got, value, delta, what, cap)
