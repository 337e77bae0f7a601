"""Shared by tests/test_frame_out_cpu.py and tests/test_gpu_frame_out.py: a numpy statement of the output
conversion of include/m2dec_amd.h, the test pictures and geometries, and the cropped coverage stream."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np

from tests._streams import GEN

FORMATS = ("nv12", "rgb", "rgbp")
MATRICES = ("bt709", "bt601")
# (matrix, full_range) -> ky, yo, rv, gu, gv, bu
COEFS = {
    ("bt601", False): (298, 16, 409, -100, -208, 516),
    ("bt709", False): (298, 16, 459, -55, -136, 541),
    ("bt601", True): (256, 0, 359, -88, -183, 454),
    ("bt709", True): (256, 0, 403, -48, -120, 475),
}
Y_VALUES = (0, 16, 17, 128, 235, 255)
C_VALUES = (0, 16, 128, 240, 255)
SIZES = ((16, 16), (32, 16), (336, 48))


def crops_for(w, h):
    """(left, right, top, bottom): none, the two mixed ones, 14 / 14 off the left and top, one leaving 2 x 2."""
    return [(0, 0, 0, 0), (2, 0, 0, 6), (6, 4, 2, 0), (14, 0, 14, 0), (2, w - 4, 2, h - 4)]


def ref_convert(luma, chroma, crop, fmt, matrix="bt709", full_range=False):
    """luma (H, W) and chroma (H / 2, W) uint8 arrays -> the cropped frame's bytes as a flat uint8 array."""
    h, w = luma.shape
    l, r, t, b = crop
    cw, ch = w - l - r, h - t - b
    if fmt == "nv12":
        return np.concatenate([luma[t:t + ch, l:l + cw].ravel(), chroma[t // 2:t // 2 + ch // 2, l:l + cw].ravel()])
    ky, yo, rv, gu, gv, bu = COEFS[(matrix, bool(full_range))]
    sy = (np.arange(ch) + t)[:, None]
    sx = (np.arange(cw) + l)[None, :]
    c = luma[sy, sx].astype(np.int32) - yo
    d = chroma[sy >> 1, (sx >> 1) * 2].astype(np.int32) - 128
    e = chroma[sy >> 1, (sx >> 1) * 2 + 1].astype(np.int32) - 128
    rr = np.clip((ky * c + rv * e + 128) >> 8, 0, 255)
    gg = np.clip((ky * c + gu * d + gv * e + 128) >> 8, 0, 255)
    bb = np.clip((ky * c + bu * d + 128) >> 8, 0, 255)
    planes = np.stack([rr, gg, bb]).astype(np.uint8)  # (3, ch, cw)
    return (planes.transpose(1, 2, 0) if fmt == "rgb" else planes).ravel()


_pictures = {}


def pictures(w, h):
    """Two (luma, chroma) pictures of w x h, built once: seeded random bytes, and random bytes with every
    (Y, Cb, Cr) of Y_VALUES x C_VALUES x C_VALUES laid over the 2 x 2 luma blocks in turn (four Y values per
    block, two blocks per chroma pair), the 50-block pattern repeated over the whole picture so that every
    crop still sees all of them where it is large enough."""
    if (w, h) in _pictures:
        return _pictures[(w, h)]
    rng = np.random.default_rng(1000 * w + h)
    rnd = (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8))
    luma = rng.integers(0, 256, (h, w), dtype=np.uint8)
    chroma = rng.integers(0, 256, (h // 2, w), dtype=np.uint8)
    ys = Y_VALUES + (Y_VALUES[0], Y_VALUES[1])  # 8 luma samples of a pair's two blocks: all 6 values
    k = 0
    for by in range(h // 2):
        for bx in range(w // 2):
            pair, half = divmod(k % 50, 2)
            chroma[by, 2 * bx] = C_VALUES[pair // 5]
            chroma[by, 2 * bx + 1] = C_VALUES[pair % 5]
            luma[2 * by:2 * by + 2, 2 * bx:2 * bx + 2] = np.array(ys[4 * half:4 * half + 4], dtype=np.uint8).reshape(2, 2)
            k += 1
    seen = {(int(luma[y, x]), int(chroma[y >> 1, x & ~1]), int(chroma[y >> 1, x | 1])) for y in range(h) for x in range(w)} \
        if w * h <= 512 else None
    if seen is not None:
        assert all((y, cb, cr) in seen for y in Y_VALUES for cb in C_VALUES for cr in C_VALUES)
    _pictures[(w, h)] = (rnd, (luma, chroma))
    return _pictures[(w, h)]


def make_frame(luma, chroma, crop):
    """An m2d_frame_t over the arrays (which the caller keeps alive)."""
    import m2dec_amd
    f = m2dec_amd.Frame()
    f.luma = luma.ctypes.data
    f.chroma = chroma.ctypes.data
    f.width, f.height = luma.shape[1], luma.shape[0]
    f.crop = (ctypes.c_int16 * 4)(*crop)
    return f


CROP_STREAM_SHA = "1931d4e8dbc47c9c"
_crop_stream = []


def crop_stream():
    """h264gen --preset cov_tools --seed 1 --frames 16 --set crop_bottom=6: 320 x 192 coded, 320 x 186 output."""
    if not _crop_stream:
        out = f"/tmp/m2dec_crop6_{os.getpid()}.264"
        subprocess.run([GEN, "--preset", "cov_tools", "--seed", "1", "--frames", "16", "--set", "crop_bottom=6", "-o", out],
                       check=True, stderr=subprocess.DEVNULL)
        data = open(out, "rb").read()
        os.unlink(out)
        assert hashlib.sha256(data).hexdigest().startswith(CROP_STREAM_SHA), "generator output drifted"
        _crop_stream.append(data)
    return _crop_stream[0]


_crop_md5 = {}


def crop_stream_oracle_md5(dpb=-1):
    """The CPU oracle's MD5 line per output frame of crop_stream() (h264dec -d dpb: -1 from the level, 1 bypass,
    which delivers in decoding order), computed once per dpb."""
    if dpb not in _crop_md5:
        import m2dec_amd
        from tests._oracle import OracleBackend
        L = m2dec_amd.lib()
        L.m2dec_amd_decode_stream2.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(m2dec_amd.Backend),
                                               ctypes.c_int, ctypes.c_int, m2dec_amd.ON_FRAME, ctypes.c_void_p,
                                               ctypes.POINTER(m2dec_amd.Stats)]
        L.m2dec_amd_decode_stream2.restype = ctypes.c_int
        got = []
        cb = m2dec_amd.ON_FRAME(lambda _a, fp: got.append(m2dec_amd.frame_md5(fp.contents)))
        data = crop_stream()
        with OracleBackend() as ob:
            n = L.m2dec_amd_decode_stream2(data, len(data), ctypes.byref(ob.be), 0, dpb, cb, None, None)
        assert n == len(got) == 16
        _crop_md5[dpb] = got
    return _crop_md5[dpb]
