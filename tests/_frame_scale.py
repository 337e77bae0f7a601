"""Shared by tests/test_frame_scale_cpu.py and tests/test_gpu_frame_scale.py: a numpy statement of the scaled and
normalised output of include/m2dec_amd.h (tap tables in Python integers, horizontal then vertical pass, element
type), its float64 evaluation, and the test geometries."""
import numpy as np

from tests._frame_out import ref_convert

ONE = 16384
MAX_TAPS = 32
FILTERS = ("bilinear", "area")
DTYPES = ("u8", "f16", "f32")
NP_DTYPE = {"u8": np.uint8, "f16": np.float16, "f32": np.float32}
ESIZE = {"u8": 1, "f16": 2, "f32": 4}
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
NORMS = (IMAGENET, ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)))

# (S, On) of the tap tests
TAP_PAIRS = ((16, 16), (16, 7), (16, 37), (62, 9), (130, 129), (318, 11), (336, 224), (48, 224), (64, 2), (1920, 224),
             (3840, 120))
# coded (w, h), crop (left, right, top, bottom), output (w, h): identity, down, up; 32 taps on both axes (area), output
# widths 2 and 1-high; a left crop of 2 mod 4 with a cropped width of 130 (no multiple of 8) and an odd output; a
# left crop of 2 with 318 columns; down in x while up in y over 7 x 28 tiles, and 2 x 2 tiles with an odd size
GEOMETRIES = (
    ((16, 16), (0, 0, 0, 0), (16, 16)),
    ((16, 16), (0, 0, 0, 0), (7, 5)),
    ((16, 16), (0, 0, 0, 0), (37, 23)),
    ((64, 32), (0, 0, 0, 0), (2, 1)),
    ((144, 16), (6, 8, 0, 0), (129, 15)),
    ((320, 16), (2, 0, 0, 0), (53, 16)),
    ((336, 48), (0, 0, 0, 0), (224, 224)),
    ((336, 48), (0, 0, 0, 0), (33, 9)),
)


def geo_id(g):
    (w, h), crop, (ow, oh) = g
    return f"{w}x{h}-{crop[0]}.{crop[1]}.{crop[2]}.{crop[3]}-{ow}x{oh}"


def _rnd(c, t):
    return (2 * c * ONE + t) // (2 * t)


def overlaps(S, On, filt, o):
    """Output o's taps as [(clamped source index, integer overlap)], merged per index, and their total T."""
    if filt == "bilinear":
        num, den = (2 * o + 1) * S - On, 2 * On
        i0 = num // den
        rem = num - i0 * den
        raw, total = [(i0, den - rem), (i0 + 1, rem)], den
    else:
        lo, hi = o * S, (o + 1) * S
        raw = [(i, min((i + 1) * On, hi) - max(i * On, lo)) for i in range(lo // On, -(-hi // On))]
        raw, total = [(i, v) for i, v in raw if v > 0], S
    merged = []
    for i, v in raw:
        i = min(max(i, 0), S - 1)
        if merged and merged[-1][0] == i:
            merged[-1] = (i, merged[-1][1] + v)
        else:
            merged.append((i, v))
    assert sum(v for _, v in merged) == total
    return merged, total


def taps(S, On, filt):
    """[(start, [weights])] per output; ValueError past MAX_TAPS."""
    out = []
    for o in range(On):
        merged, total = overlaps(S, On, filt, o)
        c, ws = 0, []
        for _, v in merged:
            ws.append(_rnd(c + v, total) - _rnd(c, total))
            c += v
        a, b = 0, len(ws)
        while not ws[a]:
            a += 1
        while not ws[b - 1]:
            b -= 1
        if b - a > MAX_TAPS:
            raise ValueError(f"{S} -> {On} ({filt}): output {o} needs {b - a} taps")
        assert [i for i, _ in merged] == list(range(merged[0][0], merged[0][0] + len(merged)))
        out.append((merged[a][0], ws[a:b]))
    return out


def tables(S, On, filt):
    """start[On], count[On], weights[On, 32] as m2dec_amd_scale_taps lays them out."""
    t = taps(S, On, filt)
    start = np.array([s for s, _ in t], np.int16)
    count = np.array([len(w) for _, w in t], np.int16)
    weights = np.zeros((On, MAX_TAPS), np.uint16)
    for o, (_, w) in enumerate(t):
        weights[o, :len(w)] = w
    return start, count, weights


_matrices = {}


def matrix(S, On, filt, exact=False):
    """The axis as a dense (On, S) matrix: the integer weights (int64), or with exact=True the float64 overlaps / T."""
    key = (S, On, filt, exact)
    if key not in _matrices:
        if exact:
            m = np.zeros((On, S), np.float64)
            for o in range(On):
                merged, total = overlaps(S, On, filt, o)
                for i, v in merged:
                    m[o, i] += v / total
        else:
            m = np.zeros((On, S), np.int64)
            for o, (s, w) in enumerate(taps(S, On, filt)):
                m[o, s:s + len(w)] = w
        _matrices[key] = m
    return _matrices[key]


def resample(planes, ow, oh, filt):
    """(3, ch, cw) uint8 -> (3, oh, ow) uint8: horizontal pass into 16 bits, then the vertical pass."""
    _, ch, cw = planes.shape
    h = (planes.astype(np.int64) @ matrix(cw, ow, filt).T + 32) >> 6  # (3, ch, ow)
    assert h.max() <= 65280
    q = (np.einsum("oy,cyx->cox", matrix(ch, oh, filt), h) + (1 << 21)) >> 22
    return np.clip(q, 0, 255).astype(np.uint8)


def resample_float(planes, ow, oh, filt):
    """The same filter evaluated in float64 with the exact weights, unrounded."""
    _, ch, cw = planes.shape
    h = planes.astype(np.float64) @ matrix(cw, ow, filt, exact=True).T
    return np.einsum("oy,cyx->cox", matrix(ch, oh, filt, exact=True), h)


def norm_coefs(mean, std):
    """(a, b) float32 per channel from float32 mean / std, computed in float64."""
    m = np.array(mean, np.float32).astype(np.float64)
    s = np.array(std, np.float32).astype(np.float64)
    return (1.0 / (255.0 * s)).astype(np.float32), (-m / s).astype(np.float32)


def normalise(q, dtype, mean, std):
    """(3, oh, ow) uint8 -> the element type: q, or float32(q a + b) evaluated in float64 (exact for the test sets:
    one rounding, as fmaf), or that float32 rounded to float16."""
    if dtype == "u8":
        return q
    a, b = norm_coefs(mean, std)
    v = (q.astype(np.float64) * a.astype(np.float64)[:, None, None] + b.astype(np.float64)[:, None, None]).astype(np.float32)
    return v if dtype == "f32" else v.astype(np.float16)


def ref_scaled(luma, chroma, crop, fmt, size=None, filt="bilinear", dtype="u8", mean=(0, 0, 0), std=(1, 1, 1),
               matrix_name="bt709", full_range=False):
    """The output frame as a flat array of the element type; size = (height, width) or None."""
    h, w = luma.shape
    cw, ch = w - crop[0] - crop[1], h - crop[2] - crop[3]
    planes = ref_convert(luma, chroma, crop, "rgbp", matrix_name, full_range).reshape(3, ch, cw)
    oh, ow = size if size is not None else (ch, cw)
    out = normalise(resample(planes, ow, oh, filt), dtype, mean, std)
    return (out.transpose(1, 2, 0) if fmt == "rgb" else out).ravel()
