"""The scaled and normalised output on the host (m2dec_amd_scale_taps, m2dec_amd_frame_convert_host with a size,
filter and element type) against the numpy statement of tests/_frame_scale.py bit for bit; its accuracy against
float64, torch's bilinear and adaptive average pooling; the refusals; the revision-6 struct; and the bounds of the
host code under AddressSanitizer in a stand-alone program."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import m2dec_amd
from tests._frame_out import make_frame, pictures, ref_convert
from tests._frame_scale import (DTYPES, FILTERS, GEOMETRIES, IMAGENET, MAX_TAPS, NORMS, NP_DTYPE, ONE, TAP_PAIRS, geo_id,
                                norm_coefs, ref_scaled, resample, resample_float, tables)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLD_DEVOUT_SIZE = 40  # revision 6: size, format, matrix, full_range, frame_dst, arg


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("pair", TAP_PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_taps_match_numpy(built, pair, filt):
    S, On = pair
    start, count, weights = m2dec_amd.scale_taps(S, On, filt)
    ws, wc, ww = tables(S, On, filt)
    assert np.array_equal(start, ws) and np.array_equal(count, wc) and np.array_equal(weights, ww)
    assert (weights.astype(np.int64).sum(axis=1) == ONE).all()
    assert (start >= 0).all() and (start.astype(np.int64) + count <= S).all()
    assert (count >= 1).all() and (count <= MAX_TAPS).all()
    for o in range(On):
        assert not weights[o, count[o]:].any()


def test_the_tap_limit(built):
    """64 -> 2 and 3840 -> 120 need exactly 32 taps; 66 -> 2 area needs 33 and is refused with nothing written."""
    assert m2dec_amd.scale_taps(64, 2, "area")[1].max() == 32
    assert m2dec_amd.scale_taps(3840, 120, "area")[1].max() == 32
    with pytest.raises(ValueError):
        tables(66, 2, "area")
    L = m2dec_amd.lib()
    start, count = np.full(2, 0x5a5a, np.int16), np.full(2, 0x5a5a, np.int16)
    weights = np.full((2, MAX_TAPS), 0xa5a5, np.uint16)
    assert L.m2dec_amd_scale_taps(66, 2, 1, start.ctypes.data, count.ctypes.data, weights.ctypes.data) == -1
    assert (start == 0x5a5a).all() and (count == 0x5a5a).all() and (weights == 0xa5a5).all()
    for S, On, f in ((0, 4, 0), (4, 0, 0), (4, 4, 2), (4, 4, -1), (16385, 4, 0), (4, 16385, 1)):
        assert L.m2dec_amd_scale_taps(S, On, f, start.ctypes.data, count.ctypes.data, weights.ctypes.data) == -1
    assert L.m2dec_amd_scale_taps(4, 2, 0, None, count.ctypes.data, weights.ctypes.data) == -1
    with pytest.raises(ValueError):
        m2dec_amd.scale_taps(66, 2, "area")
    assert m2dec_amd.scale_taps(66, 2, "bilinear")[1].max() <= 2  # (two taps at the most: never refused)


@pytest.mark.parametrize("geo", GEOMETRIES, ids=geo_id)
def test_host_model_matches_numpy(built, geo):
    (w, h), crop, (ow, oh) = geo
    mean, std = IMAGENET
    n = 0
    for luma, chroma in pictures(w, h):
        f = make_frame(luma, chroma, crop)
        for filt in FILTERS:
            for fmt in ("rgb", "rgbp"):
                for dtype in DTYPES:
                    raw = m2dec_amd.frame_convert_host(f, fmt, size=(oh, ow), filter=filt, dtype=dtype, mean=mean, std=std)
                    got = np.frombuffer(raw, dtype=NP_DTYPE[dtype])
                    want = ref_scaled(luma, chroma, crop, fmt, (oh, ow), filt, dtype, mean, std)
                    assert got.shape == want.shape == (3 * ow * oh,), (geo, filt, fmt, dtype)
                    assert got.tobytes() == want.tobytes(), (geo, filt, fmt, dtype)
                    n += 1
    assert n == 2 * 12


def test_other_matrix_and_range_reach_the_scaled_path(built):
    (w, h), crop, (ow, oh) = GEOMETRIES[4]
    luma, chroma = pictures(w, h)[1]
    f = make_frame(luma, chroma, crop)
    raw = m2dec_amd.frame_convert_host(f, "rgb", "bt601", True, size=(oh, ow), filter="area")
    want = ref_scaled(luma, chroma, crop, "rgb", (oh, ow), "area", matrix_name="bt601", full_range=True)
    assert raw == want.tobytes()


@pytest.mark.parametrize("geo", GEOMETRIES[:1] + GEOMETRIES[4:7], ids=geo_id)
def test_identity_returns_the_unscaled_bytes(built, geo):
    (w, h), crop, _ = geo
    cw, ch = w - crop[0] - crop[1], h - crop[2] - crop[3]
    for luma, chroma in pictures(w, h):
        f = make_frame(luma, chroma, crop)
        for fmt in ("rgb", "rgbp"):
            plain = m2dec_amd.frame_convert_host(f, fmt)
            assert plain == ref_convert(luma, chroma, crop, fmt).tobytes()
            for filt in FILTERS:
                assert m2dec_amd.frame_convert_host(f, fmt, size=(ch, cw), filter=filt) == plain, (geo, fmt, filt)


@pytest.mark.parametrize("geo", GEOMETRIES, ids=geo_id)
def test_within_one_of_the_float64_filter(built, geo):
    """The bound of 1, derived: the vertical pass rounds to within 1/2, the horizontal one to within 1/512 (its unit
    is 1/256), and per axis the running sums of the weights are within 2^-15 of the exact ones, which by summation
    by parts moves a weighted sum of up to 32 samples by at most 31 * 255 * 2^-15 < 0.242:
    |fixed - float64| < 0.5 + 0.002 + 2 * 0.242 < 1."""
    (w, h), crop, (ow, oh) = geo
    cw, ch = w - crop[0] - crop[1], h - crop[2] - crop[3]
    for luma, chroma in pictures(w, h):
        planes = ref_convert(luma, chroma, crop, "rgbp").reshape(3, ch, cw)
        f = make_frame(luma, chroma, crop)
        for filt in FILTERS:
            got = np.frombuffer(m2dec_amd.frame_convert_host(f, "rgbp", size=(oh, ow), filter=filt), np.uint8)
            err = np.abs(got.reshape(3, oh, ow).astype(np.float64) - resample_float(planes, ow, oh, filt)).max()
            print(f"{geo_id(geo)} {filt}: max |fixed - float64| = {err:.4f}")
            assert err <= 1.0, (geo, filt, err)


TORCH_CODE = """
import sys
import numpy as np
import torch
import torch.nn.functional as F
import m2dec_amd
from tests._frame_out import make_frame, pictures, ref_convert
from tests._frame_scale import GEOMETRIES
worst = 0.0
for (w, h), crop, (ow, oh) in GEOMETRIES:
    cw, ch = w - crop[0] - crop[1], h - crop[2] - crop[3]
    for luma, chroma in pictures(w, h):
        planes = ref_convert(luma, chroma, crop, "rgbp").reshape(1, 3, ch, cw)
        want = F.interpolate(torch.from_numpy(planes.astype(np.float64)), size=(oh, ow), mode="bilinear",
                             align_corners=False, antialias=False).numpy()[0]
        got = np.frombuffer(m2dec_amd.frame_convert_host(make_frame(luma, chroma, crop), "rgbp", size=(oh, ow),
                                                         filter="bilinear"), np.uint8).reshape(3, oh, ow)
        err = float(np.abs(got.astype(np.float64) - want).max())
        print("bilinear", (w, h), crop, (ow, oh), err)
        worst = max(worst, err)
        assert err <= 1.0, ("bilinear", (w, h), crop, (ow, oh), err)
# area at integer ratios: adaptive_avg_pool2d
for (w, h), (ow, oh) in (((16, 16), (4, 8)), ((64, 32), (2, 1)), ((336, 48), (112, 16)), ((336, 48), (336, 48))):
    for luma, chroma in pictures(w, h):
        planes = ref_convert(luma, chroma, (0, 0, 0, 0), "rgbp").reshape(1, 3, h, w)
        want = F.adaptive_avg_pool2d(torch.from_numpy(planes.astype(np.float64)), (oh, ow)).numpy()[0]
        got = np.frombuffer(m2dec_amd.frame_convert_host(make_frame(luma, chroma, (0, 0, 0, 0)), "rgbp", size=(oh, ow),
                                                         filter="area"), np.uint8).reshape(3, oh, ow)
        err = float(np.abs(got.astype(np.float64) - want).max())
        print("area", (w, h), (ow, oh), err)
        assert err <= 1.0, ("area", (w, h), (ow, oh), err)
print("TORCH_OK", worst)
"""


def test_within_one_of_torch_bilinear_and_adaptive_avg_pool(built):
    """CPU torch, in a process of its own with torch imported first (torch wheels carry their own HIP runtime: see
    test_gpu_frame_out.test_torch_adopts_the_frames)."""
    pytest.importorskip("torch")
    r = subprocess.run([sys.executable, "-c", TORCH_CODE], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("TORCH_OK"), r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.parametrize("norm", NORMS, ids=["imagenet", "unit", "half"])
def test_normalisation_is_one_fma(built, norm):
    mean, std = norm
    (w, h), crop, (ow, oh) = GEOMETRIES[5]
    cw, ch = w - crop[0] - crop[1], h - crop[2] - crop[3]
    a, b = norm_coefs(mean, std)
    for luma, chroma in pictures(w, h):
        f = make_frame(luma, chroma, crop)
        q = resample(ref_convert(luma, chroma, crop, "rgbp").reshape(3, ch, cw), ow, oh, "area")
        exact = q.astype(np.float64) * a.astype(np.float64)[:, None, None] + b.astype(np.float64)[:, None, None]
        want32 = exact.astype(np.float32)
        got32 = np.frombuffer(m2dec_amd.frame_convert_host(f, "rgbp", size=(oh, ow), filter="area", dtype="f32", mean=mean,
                                                           std=std), np.float32).reshape(3, oh, ow)
        assert got32.tobytes() == want32.tobytes()
        got16 = np.frombuffer(m2dec_amd.frame_convert_host(f, "rgbp", size=(oh, ow), filter="area", dtype="f16", mean=mean,
                                                           std=std), np.float16).reshape(3, oh, ow)
        assert got16.tobytes() == want32.astype(np.float16).tobytes()
        if norm == NORMS[1]:
            # plain q / 255, to float32's precision (a = float32(1 / 255) carries half an ulp of its own)
            assert np.allclose(got32, q.astype(np.float64) / 255.0, rtol=2.0 ** -22, atol=0)
    # every q, unscaled float output included: a 16 x 16 picture's 256 luma values on grey chroma, full range
    luma = np.arange(256, dtype=np.uint8).reshape(16, 16)
    chroma = np.full((8, 16), 128, np.uint8)
    f = make_frame(luma, chroma, (0, 0, 0, 0))
    got = np.frombuffer(m2dec_amd.frame_convert_host(f, "rgbp", "bt601", True, dtype="f32", mean=mean, std=std), np.float32)
    qs = np.arange(256, dtype=np.float64)
    for c in range(3):
        assert got[256 * c:256 * (c + 1)].tobytes() == (qs * np.float64(a[c]) + np.float64(b[c])).astype(np.float32).tobytes()


def _cfg(**kw):
    args = dict(size=ctypes.sizeof(m2dec_amd.DevOut), format=1, matrix=0, full_range=0, out_width=8, out_height=8, filter=0,
                dtype=0, mean=(ctypes.c_float * 3)(0, 0, 0), std=(ctypes.c_float * 3)(1, 1, 1))
    args.update(kw)
    for k in ("mean", "std"):
        args[k] = (ctypes.c_float * 3)(*args[k])
    return m2dec_amd.DevOut(**args)


INF, NAN = float("inf"), float("nan")
REFUSED = {
    "nv12_scaled": dict(format=0),
    "nv12_f32": dict(format=0, out_width=0, out_height=0, dtype=2),
    "nv12_f16": dict(format=0, out_width=0, out_height=0, dtype=1),
    "width_negative": dict(out_width=-1),
    "height_negative": dict(out_height=-8),
    "only_width": dict(out_height=0),
    "only_height": dict(out_width=0),
    "filter_2": dict(filter=2),
    "filter_negative": dict(filter=-1),
    "dtype_3": dict(dtype=3),
    "dtype_negative": dict(dtype=-1),
    "std_zero": dict(dtype=2, std=(1, 0, 1)),
    "std_negative": dict(dtype=1, std=(-1, 1, 1)),
    "std_inf": dict(dtype=2, std=(1, 1, INF)),
    "std_nan": dict(dtype=2, std=(NAN, 1, 1)),
    "mean_inf": dict(dtype=2, mean=(0, INF, 0)),
    "mean_nan": dict(dtype=1, mean=(0, 0, NAN)),
    "taps_33_x": dict(out_width=2, out_height=8, filter=1),   # 66 -> 2
    "taps_33_y": dict(out_width=8, out_height=1, filter=1),   # 34 -> 1
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusals_write_nothing(built, name):
    luma, chroma = pictures(80, 48)[0]
    f = make_frame(luma, chroma, (14, 0, 14, 0))  # 66 x 34
    L = m2dec_amd.lib()
    cfg = _cfg(**REFUSED[name])
    out = ctypes.create_string_buffer(b"\xa5" * 32768, 32768)
    assert L.m2dec_amd_frame_convert_host(ctypes.byref(f), ctypes.byref(cfg), out) == -1
    assert out.raw == b"\xa5" * 32768
    assert L.m2dec_amd_frame_out_bytes2(ctypes.byref(cfg), 66, 34, None, None) == 0
    # the same config made valid converts (the refusal is this field's)
    ok = _cfg()
    assert L.m2dec_amd_frame_out_bytes2(ctypes.byref(ok), 66, 34, None, None) == 8 * 8 * 3
    assert L.m2dec_amd_frame_convert_host(ctypes.byref(f), ctypes.byref(ok), out) == 0


@pytest.mark.parametrize("kw", [
    dict(fmt="nv12", size=(8, 8)), dict(fmt="nv12", dtype="f32"), dict(size=(0, 8)), dict(size=(8, -1)), dict(size=(8,)),
    dict(size=8), dict(filter="bicubic"), dict(dtype="f64"), dict(dtype="f32", std=(1, 0, 1)), dict(dtype="f16", std=(1, 1, INF)),
    dict(dtype="f32", mean=(NAN, 0, 0)), dict(dtype="f32", mean=(0, 0)), dict(size=(1, 2), filter="area"),
    dict(size=(20000, 8)),
], ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_python_raises_value_error(built, kw):
    luma, chroma = pictures(80, 48)[0]
    f = make_frame(luma, chroma, (14, 0, 14, 0))
    with pytest.raises(ValueError):
        m2dec_amd.frame_convert_host(f, **kw)
    if kw.get("size") != (1, 2):  # (33 taps: known only with the picture's size)
        # the stream entry checks its arguments before any GPU work: no device is needed to be refused
        with pytest.raises(ValueError):
            m2dec_amd.decode_to_device(b"", **kw)
    with pytest.raises(ValueError):
        m2dec_amd.hip_frame_convert(luma.tobytes(), chroma.tobytes(), 80, 48, (14, 0, 14, 0), **kw)


def test_misaligned_float_offset_is_a_value_error(built):
    luma, chroma = pictures(16, 16)[0]
    for dtype, off in (("f16", 1), ("f32", 2), ("f32", 1)):
        with pytest.raises(ValueError):
            m2dec_amd.hip_frame_convert(luma.tobytes(), chroma.tobytes(), 16, 16, dtype=dtype, out_offset=off)


def test_revision_6_struct_converts_unscaled(built):
    """A caller that passes the old struct size: the trailing fields are not read, whatever they hold."""
    assert ctypes.sizeof(m2dec_amd.DevOut) == 80
    luma, chroma = pictures(16, 16)[1]
    f = make_frame(luma, chroma, (2, 0, 0, 6))
    L = m2dec_amd.lib()
    for fmt in ("nv12", "rgb", "rgbp"):
        cfg = _cfg(size=OLD_DEVOUT_SIZE, format=m2dec_amd.OUT_FORMATS[fmt], out_width=-3, out_height=7, filter=9, dtype=5,
                   std=(0, 0, 0))
        want = ref_convert(luma, chroma, (2, 0, 0, 6), fmt).tobytes()
        ow, oh = ctypes.c_int(), ctypes.c_int()
        assert L.m2dec_amd_frame_out_bytes2(ctypes.byref(cfg), 14, 10, ctypes.byref(ow), ctypes.byref(oh)) == len(want)
        assert (ow.value, oh.value) == (14, 10)
        out = ctypes.create_string_buffer(len(want))
        assert L.m2dec_amd_frame_convert_host(ctypes.byref(f), ctypes.byref(cfg), out) == 0
        assert out.raw == want
    # and the new fields at zero are today's path too
    cfg = m2dec_amd.DevOut(size=ctypes.sizeof(m2dec_amd.DevOut), format=1, matrix=0, full_range=0)
    out = ctypes.create_string_buffer(14 * 10 * 3)
    assert L.m2dec_amd_frame_convert_host(ctypes.byref(f), ctypes.byref(cfg), out) == 0
    assert out.raw == ref_convert(luma, chroma, (2, 0, 0, 6), "rgb").tobytes()
    assert L.m2dec_amd_abi_version() == 7


def test_host_code_bounds_under_address_sanitizer(built, tmp_path):
    """tests/harness/frame_scale_bounds.c with frame_out.c, -fsanitize=address,undefined, as a child process: every
    plane, table and output an exact-size malloc."""
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "frame_scale_bounds")
    # (the sanitizer runtimes linked statically: the program then runs whatever else the loader brings in first)
    cmd = [cc, "-O1", "-g", "-std=gnu11", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "m2dec_amd", "csrc", "host"), "-o", exe,
           os.path.join(ROOT, "tests", "harness", "frame_scale_bounds.c"),
           os.path.join(ROOT, "m2dec_amd", "csrc", "host", "frame_out.c"), "-lm"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and r.stdout.startswith("BOUNDS_OK"), r.stdout[-1000:] + r.stderr[-3000:]
