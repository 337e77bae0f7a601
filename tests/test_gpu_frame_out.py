"""Device-resident H.264 output on the GPU: k_frame_out against the host restatement bit for bit, whole streams
decoded into device memory against their golden MD5s, the RGB forms against numpy, both ways a picture reaches a
frame slot, and the memory handed to other libraries."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

import m2dec_amd
from tests._frame_out import (FORMATS, MATRICES, SIZES, crop_stream, crop_stream_oracle_md5, crops_for, make_frame,
                              pictures, ref_convert)
from tests._oracle import golden_md5s
from tests._streams import GOLDEN, stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = b"\xa5" * 64

# coded size, crops: the CPU test's list, then cropped widths 62, 130 and 318 (a partial last patch of 6 columns,
# 2 and 6 again) with the left crop a multiple of 4, 2 mod 4, and none
GEOMETRIES = [(s, crops_for(*s)) for s in SIZES] + [
    ((64, 16), [(0, 2, 0, 0), (2, 0, 0, 0)]),
    ((144, 16), [(6, 8, 0, 0), (8, 6, 2, 2)]),
    ((320, 16), [(2, 0, 0, 0), (0, 2, 0, 0)]),
]


@pytest.mark.gpu
@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: f"{g[0][0]}x{g[0][1]}")
def test_kernel_matches_host_restatement(built, geo):
    (w, h), crops = geo
    for luma, chroma in pictures(w, h):
        lb, cb = luma.tobytes(), chroma.tobytes()
        for crop in crops:
            f = make_frame(luma, chroma, crop)
            for fmt in FORMATS:
                for matrix in MATRICES:
                    for full in (False, True):
                        want = m2dec_amd.frame_convert_host(f, fmt, matrix, full)
                        for off in (0, 1, 3):
                            got, before, after = m2dec_amd.hip_frame_convert(lb, cb, w, h, crop, fmt, matrix, full,
                                                                             out_offset=off)
                            where = (w, h, crop, fmt, matrix, full, off)
                            assert before == GUARD and after == GUARD, where
                            assert got == want, where


@pytest.mark.gpu
def test_kernel_entry_refuses_odd_crops(built):
    (luma, chroma), _ = pictures(16, 16)
    for crop in ((1, 0, 0, 0), (0, 0, 3, 0), (8, 8, 0, 0)):
        with pytest.raises((RuntimeError, ValueError)):
            m2dec_amd.hip_frame_convert(luma.tobytes(), chroma.tobytes(), 16, 16, crop, "rgb")


def _md5s(arr):
    return [hashlib.md5(arr[i].tobytes()).hexdigest() for i in range(arr.shape[0])]


def _stream_and_golden(name):
    if name == "crop6":
        return crop_stream(), crop_stream_oracle_md5(), (320, 186)
    if name == "f1":
        data = open(os.path.join(ROOT, "tests", "golden", "f1_realshort.264"), "rb").read()
        return data, golden_md5s(os.path.join(ROOT, "tests", "golden", "f1_realshort.md5")), (320, 240)
    return stream(name), GOLDEN[name]["md5"], (320, 192)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cov_tools_s1", "crop6", "f1"])
def test_decode_to_device_nv12_matches_golden(built, name):
    data, want, (w, h) = _stream_and_golden(name)
    st = m2dec_amd.Stats()
    with m2dec_amd.decode_to_device(data, fmt="nv12", stats=st) as fr:
        assert fr.shape == (len(want), h * 3 // 2, w)
        got = _md5s(fr.numpy())
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert len(got) == len(want) and not bad, f"{name}: frames {bad[:10]} differ (of {len(want)})"
    assert st.frames_out == len(want) and st.d2h_bytes == 0 and st.host_copy_us == 0


@pytest.fixture(scope="module")
def crop6_nv12(built):
    """The cropped stream's frames as NV12 from the device, once: (16, 279, 320)."""
    with m2dec_amd.decode_to_device(crop_stream(), fmt="nv12") as fr:
        return fr.numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("matrix,full", [("bt709", False), ("bt601", True)], ids=["bt709_limited", "bt601_full"])
@pytest.mark.parametrize("fmt", ["rgb", "rgbp"])
def test_rgb_frames_match_numpy_of_the_nv12_frames(built, crop6_nv12, fmt, matrix, full):
    w, h = 320, 186
    with m2dec_amd.decode_to_device(crop_stream(), fmt=fmt, matrix=matrix, full_range=full) as fr:
        assert fr.shape == ((16, h, w, 3) if fmt == "rgb" else (16, 3, h, w))
        got = fr.numpy()
    assert _md5s(crop6_nv12) == crop_stream_oracle_md5()
    for i in range(16):
        luma = crop6_nv12[i, :h]
        chroma = crop6_nv12[i, h:]
        want = ref_convert(luma, chroma, (0, 0, 0, 0), fmt, matrix, full)
        assert np.array_equal(got[i].ravel(), want), (fmt, matrix, full, i)


@pytest.mark.gpu
@pytest.mark.parametrize("env,dpb", [({"M2DEC_AMD_PARSE_THREADS": "0"}, -1), ({"M2DEC_AMD_PRESTAGE": "0"}, -1), ({}, 1)],
                         ids=["direct_path", "copy_at_bind", "dpb_bypass"])
def test_device_output_on_every_path(built, monkeypatch, env, dpb):
    """The direct path (no parse-ahead: the caller's slot is the picture buffer), the decode-ahead path with the
    staging copy issued at bind, and DPB bypass (env read when the decode's back end is created)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    st = m2dec_amd.Stats()
    with m2dec_amd.decode_to_device(crop_stream(), fmt="nv12", dpb=dpb, stats=st) as fr:
        got = _md5s(fr.numpy())
    # (bypass delivers in decoding order: the oracle's list is taken with the same dpb)
    assert got == crop_stream_oracle_md5(dpb)
    if dpb == 1:
        assert got != crop_stream_oracle_md5() and sorted(got) == sorted(crop_stream_oracle_md5())
    if "M2DEC_AMD_PARSE_THREADS" in env:
        assert st.ahead == 0
    assert st.d2h_bytes == 0


@pytest.mark.gpu
def test_no_host_traffic_and_no_leak_into_other_back_ends(built):
    name = "cov_tools_s1"
    st = m2dec_amd.Stats()
    with m2dec_amd.decode_to_device(stream(name), fmt="rgb", stats=st) as fr:
        assert len(fr) == len(GOLDEN[name]["md5"])
    assert st.d2h_bytes == 0 and st.host_copy_us == 0 and st.d2h_us == 0
    assert st.frames_out == len(GOLDEN[name]["md5"])
    st2 = m2dec_amd.Stats()
    assert m2dec_amd.decode_stream_md5(stream(name), stats=st2) == GOLDEN[name]["md5"]
    assert st2.d2h_bytes == 320 * 192 * 3 // 2 * len(GOLDEN[name]["md5"])
    assert m2dec_amd.decode_stream_md5(crop_stream()) == crop_stream_oracle_md5()


@pytest.mark.gpu
def test_frame_dst_returning_null_ends_the_decode(built):
    L = m2dec_amd.lib()
    calls = []

    def dst(_arg, index, w, h, n):
        calls.append((index, w, h, n))
        return None

    cfg = m2dec_amd.DevOut(size=ctypes.sizeof(m2dec_amd.DevOut), format=0, matrix=0, full_range=0)
    cfg.frame_dst = m2dec_amd.FRAME_DST(dst)
    data = crop_stream()
    assert L.m2dec_amd_decode_stream_device(data, len(data), 0, -1, ctypes.byref(cfg), None) == -1
    assert calls == [(0, 320, 186, 320 * 186 * 3 // 2)]


@pytest.mark.gpu
def test_cuda_array_interface(built):
    with m2dec_amd.decode_to_device(crop_stream(), fmt="rgbp") as fr:
        cai = fr.__cuda_array_interface__
        assert cai["version"] == 3 and cai["typestr"] == "|u1" and cai["shape"] == (16, 3, 186, 320) == fr.shape
        assert cai["data"] == (fr.ptr, False) and fr.ptr and cai.get("strides") is None
    assert fr.ptr is None
    with pytest.raises(RuntimeError):
        fr.__cuda_array_interface__


TORCH_CODE = """
import torch
torch.cuda.init()  # torch's HIP runtime is the process's one copy: loaded before the library asks for the same soname
import numpy as np
import m2dec_amd
from tests._frame_out import crop_stream
with m2dec_amd.decode_to_device(crop_stream(), fmt="rgb") as fr:
    host = fr.numpy()
    t = torch.as_tensor(fr, device="cuda:0")
    assert tuple(t.shape) == fr.shape == (16, 186, 320, 3) and t.dtype == torch.uint8 and t.data_ptr() == fr.ptr
    assert np.array_equal(t.cpu().numpy(), host) and host.any()
    del t
print("TORCH_OK")
"""


@pytest.mark.gpu
def test_torch_adopts_the_frames(built):
    """torch.as_tensor(frames, device="cuda:0") over __cuda_array_interface__ equals frames.numpy().  In a process
    of its own with torch imported first: torch wheels carry their own libamdhip64 (soname libamdhip64.so.7, asked
    for as libamdhip64.so), so a process in which the library's runtime was loaded first ends up with two copies,
    and torch's then finds no device (seen on an MI355X: "No HIP GPUs are available"); loaded first, torch's copy
    also serves the library."""
    pytest.importorskip("torch")
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-c", TORCH_CODE], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and r.stdout.strip().endswith("TORCH_OK"), r.stdout[-1000:] + r.stderr[-3000:]
