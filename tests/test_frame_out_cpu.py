"""The output conversion on the host (m2dec_amd_frame_convert_host) against a numpy statement of the same integer
arithmetic, bit for bit: every format, matrix and range, over crops that misalign the source and leave partial
patches; and its NV12 form against the MD5 lines FileWriterMd5 would write."""
import ctypes
import hashlib

import numpy as np
import pytest

import m2dec_amd
from tests._frame_out import (FORMATS, MATRICES, SIZES, crop_stream, crop_stream_oracle_md5, crops_for, make_frame,
                              pictures, ref_convert)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_conversion_matches_numpy(built, size):
    w, h = size
    n = 0
    for luma, chroma in pictures(w, h):
        for crop in crops_for(w, h):
            f = make_frame(luma, chroma, crop)
            for fmt in FORMATS:
                for matrix in MATRICES:
                    for full in (False, True):
                        got = np.frombuffer(m2dec_amd.frame_convert_host(f, fmt, matrix, full), dtype=np.uint8)
                        want = ref_convert(luma, chroma, crop, fmt, matrix, full)
                        assert got.shape == want.shape and np.array_equal(got, want), (size, crop, fmt, matrix, full)
                        n += 1
    assert n == 2 * 5 * 12


def test_shapes_of_the_smallest_frame(built):
    (luma, chroma), _ = pictures(16, 16)
    f = make_frame(luma, chroma, (14, 0, 14, 0))
    assert len(m2dec_amd.frame_convert_host(f, "nv12")) == 6
    assert len(m2dec_amd.frame_convert_host(f, "rgb")) == 12
    assert len(m2dec_amd.frame_convert_host(f, "rgbp")) == 12


@pytest.mark.parametrize("crop", [(1, 0, 0, 0), (0, 3, 0, 0), (0, 0, 5, 0), (0, 0, 0, 7), (8, 8, 0, 0), (0, 0, 16, 0)])
def test_odd_or_empty_crop_is_refused_and_writes_nothing(built, crop):
    (luma, chroma), _ = pictures(16, 16)
    f = make_frame(luma, chroma, crop)
    L = m2dec_amd.lib()
    for fmt in FORMATS:
        cfg = m2dec_amd.DevOut(size=ctypes.sizeof(m2dec_amd.DevOut), format=m2dec_amd.OUT_FORMATS[fmt], matrix=0, full_range=0)
        out = ctypes.create_string_buffer(b"\xa5" * 1024, 1024)
        assert L.m2dec_amd_frame_convert_host(ctypes.byref(f), ctypes.byref(cfg), out) == -1
        assert out.raw == b"\xa5" * 1024
        with pytest.raises(ValueError):
            m2dec_amd.frame_convert_host(f, fmt)


def test_bad_config_is_refused(built):
    (luma, chroma), _ = pictures(16, 16)
    f = make_frame(luma, chroma, (0, 0, 0, 0))
    L = m2dec_amd.lib()
    out = ctypes.create_string_buffer(1024)
    for kw in ({"format": 3}, {"format": -1}, {"matrix": 2}, {"size": 8}):
        args = {"size": ctypes.sizeof(m2dec_amd.DevOut), "format": 1, "matrix": 0, "full_range": 0}
        args.update(kw)
        cfg = m2dec_amd.DevOut(**args)
        assert L.m2dec_amd_frame_convert_host(ctypes.byref(f), ctypes.byref(cfg), out) == -1, kw


def test_nv12_bytes_are_what_the_md5_writer_hashes(built):
    """Every frame of the cropped coverage stream (320 x 192 coded, bottom crop 6 -> 320 x 186, 93 chroma rows)
    through the CPU oracle: md5(convert(frame, nv12)) is the frame's MD5 line."""
    from tests._oracle import OracleBackend
    got = []

    def on_frame(f):
        assert (f.width, f.height, tuple(f.crop)) == (320, 192, (0, 0, 0, 6))
        nv12 = m2dec_amd.frame_convert_host(f, "nv12")
        assert len(nv12) == 320 * 186 * 3 // 2
        got.append((hashlib.md5(nv12).hexdigest(), m2dec_amd.frame_md5(f)))

    with OracleBackend() as ob:
        lines = m2dec_amd.decode_stream(crop_stream(), backend=ob.be, on_frame=on_frame)
    assert len(got) == 16 and len(lines) == 16
    assert [a for a, _ in got] == [b for _, b in got] == lines == crop_stream_oracle_md5()
