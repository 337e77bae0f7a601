"""The scaled and normalised device output on the GPU: k_frame_scale against the host model bit for bit with both
guards intact, the kernel entry's refusals, whole streams decoded into resized uint8 / float16 frames against the
numpy statement of their NV12 frames, the float16 memory handed to torch, and the back ends that run afterwards."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import m2dec_amd
from tests._frame_out import crop_stream, crop_stream_oracle_md5, make_frame, pictures
from tests._frame_scale import DTYPES, ESIZE, FILTERS, GEOMETRIES, IMAGENET, NP_DTYPE, geo_id, ref_scaled
from tests._streams import GOLDEN, stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = b"\xa5" * 64


def _md5s(arr):
    return [hashlib.md5(arr[i].tobytes()).hexdigest() for i in range(arr.shape[0])]


@pytest.mark.gpu
@pytest.mark.parametrize("geo", GEOMETRIES, ids=geo_id)
def test_kernel_matches_host_model(built, geo):
    (w, h), crop, (ow, oh) = geo
    mean, std = IMAGENET
    for luma, chroma in pictures(w, h):
        lb, cb = luma.tobytes(), chroma.tobytes()
        f = make_frame(luma, chroma, crop)
        for filt in FILTERS:
            for fmt in ("rgb", "rgbp"):
                for dtype in DTYPES:
                    want = m2dec_amd.frame_convert_host(f, fmt, size=(oh, ow), filter=filt, dtype=dtype, mean=mean, std=std)
                    for k in (0, 1, 3):
                        off = k * ESIZE[dtype]
                        got, before, after = m2dec_amd.hip_frame_convert(lb, cb, w, h, crop, fmt, out_offset=off,
                                                                         size=(oh, ow), filter=filt, dtype=dtype,
                                                                         mean=mean, std=std)
                        where = (geo, filt, fmt, dtype, off)
                        assert before == GUARD and after == GUARD, where
                        assert got == want, where


@pytest.mark.gpu
def test_unscaled_float_output_and_other_matrix(built):
    """No size with a float dtype takes k_frame_scale with identity taps; BT.601 full range reaches it too."""
    w, h, crop = 144, 16, (6, 8, 0, 0)
    luma, chroma = pictures(w, h)[1]
    f = make_frame(luma, chroma, crop)
    for kw in (dict(dtype="f32"), dict(dtype="f16", mean=IMAGENET[0], std=IMAGENET[1]),
               dict(size=(15, 129), filter="area", matrix="bt601", full_range=True)):
        for fmt in ("rgb", "rgbp"):
            want = m2dec_amd.frame_convert_host(f, fmt, **kw)
            got, before, after = m2dec_amd.hip_frame_convert(luma.tobytes(), chroma.tobytes(), w, h, crop, fmt, **kw)
            assert before == GUARD and after == GUARD and got == want, (kw, fmt)


@pytest.mark.gpu
def test_kernel_entry_refusals_launch_nothing(built):
    import ctypes
    L = m2dec_amd.lib()
    luma, chroma = pictures(80, 48)[0]
    lb, cb = luma.tobytes(), chroma.tobytes()
    crop = (ctypes.c_int16 * 4)(14, 0, 14, 0)  # 66 x 34
    three = ctypes.c_float * 3

    def cfg(**kw):
        args = dict(size=ctypes.sizeof(m2dec_amd.DevOut), format=1, matrix=0, full_range=0, out_width=8, out_height=8,
                    filter=0, dtype=0, mean=three(0, 0, 0), std=three(1, 1, 1))
        args.update(kw)
        return m2dec_amd.DevOut(**args)

    cases = {"f32 at offset 2": (cfg(dtype=2), 2), "f16 at offset 1": (cfg(dtype=1), 1), "nv12 scaled": (cfg(format=0), 0),
             "33 taps": (cfg(out_width=2, filter=1), 0)}
    for name, (c, off) in cases.items():
        out = ctypes.create_string_buffer(b"\x5a" * 4096, 4096)
        assert L.m2dec_amd_hip_frame_convert(0, lb, cb, 80, 48, crop, ctypes.byref(c), out, off) == -1, name
        assert out.raw == b"\x5a" * 4096, name
    out = ctypes.create_string_buffer(8 * 8 * 3 + 128)
    assert L.m2dec_amd_hip_frame_convert(0, lb, cb, 80, 48, crop, ctypes.byref(cfg()), out, 0) == 0
    with pytest.raises(ValueError):
        m2dec_amd.hip_frame_convert(lb, cb, 80, 48, (14, 0, 14, 0), size=(8, 2), filter="area")


@pytest.fixture(scope="module")
def crop6_nv12(built):
    """The cropped stream's frames as NV12 from the device, once per delivery order: (16, 279, 320)."""
    cache = {}

    def get(dpb=-1):
        if dpb not in cache:
            with m2dec_amd.decode_to_device(crop_stream(), fmt="nv12", dpb=dpb) as fr:
                cache[dpb] = fr.numpy()
            assert _md5s(cache[dpb]) == crop_stream_oracle_md5(dpb)
        return cache[dpb]

    return get


SCALED = {
    "area_f16_rgbp": dict(fmt="rgbp", size=(93, 160), filter="area", dtype="f16", mean=IMAGENET[0], std=IMAGENET[1]),
    "bilinear_u8_rgb": dict(fmt="rgb", size=(200, 333), filter="bilinear", dtype="u8"),
}


def _check_scaled_decode(nv12, kw, dpb=-1):
    w, h = 320, 186
    oh, ow = kw["size"]
    st = m2dec_amd.Stats()
    with m2dec_amd.decode_to_device(crop_stream(), dpb=dpb, stats=st, **kw) as fr:
        assert fr.shape == ((16, oh, ow, 3) if kw["fmt"] == "rgb" else (16, 3, oh, ow))
        got = fr.numpy()
    assert got.dtype == NP_DTYPE[kw["dtype"]]
    assert st.d2h_bytes == 0 and st.host_copy_us == 0 and st.frames_out == 16
    for i in range(16):
        want = ref_scaled(nv12[i, :h], nv12[i, h:], (0, 0, 0, 0), kw["fmt"], kw["size"], kw["filter"], kw["dtype"],
                          kw.get("mean", (0, 0, 0)), kw.get("std", (1, 1, 1)))
        assert got[i].tobytes() == want.tobytes(), (kw, i)
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCALED))
def test_scaled_stream_matches_numpy_of_the_nv12_frames(built, crop6_nv12, name):
    _check_scaled_decode(crop6_nv12(), SCALED[name])


@pytest.mark.gpu
@pytest.mark.parametrize("env,dpb", [({"M2DEC_AMD_PARSE_THREADS": "0"}, -1), ({}, 1)], ids=["direct_path", "dpb_bypass"])
def test_scaled_stream_on_the_other_paths(built, crop6_nv12, monkeypatch, env, dpb):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    nv12 = crop6_nv12(dpb)
    st = _check_scaled_decode(nv12, SCALED["area_f16_rgbp"], dpb)
    if env:
        assert st.ahead == 0


@pytest.mark.gpu
def test_stream_driver_takes_the_revision_6_struct_and_passes_the_output_size(built):
    """frame_dst is asked for frame 0 (and ends the decode by answering NULL): with the old struct size, whatever
    the trailing fields hold, for the cropped NV12 frame; with the new fields, for the output size and bytes."""
    import ctypes
    L = m2dec_amd.lib()
    calls = []

    def dst(_arg, index, w, h, n):
        calls.append((index, w, h, n))
        return None

    data = crop_stream()
    three = ctypes.c_float * 3
    old = m2dec_amd.DevOut(size=40, format=0, matrix=0, full_range=0, out_width=-5, out_height=3, filter=7, dtype=9)
    new = m2dec_amd.DevOut(size=ctypes.sizeof(m2dec_amd.DevOut), format=2, matrix=0, full_range=0, out_width=160,
                           out_height=93, filter=1, dtype=1, mean=three(0, 0, 0), std=three(1, 1, 1))
    bad = m2dec_amd.DevOut(size=ctypes.sizeof(m2dec_amd.DevOut), format=2, matrix=0, full_range=0, out_width=160,
                           out_height=0)
    for cfg in (old, new, bad):
        cfg.frame_dst = m2dec_amd.FRAME_DST(dst)
        assert L.m2dec_amd_decode_stream_device(data, len(data), 0, -1, ctypes.byref(cfg), None) == -1
    # (the refused config ends the decode before frame_dst is asked)
    assert calls == [(0, 320, 186, 320 * 186 * 3 // 2), (0, 160, 93, 160 * 93 * 3 * 2)]


@pytest.mark.gpu
def test_scale_launches_are_timed_like_frame_out(built):
    m2dec_amd.frame_out_timing(reset=True)
    with m2dec_amd.decode_to_device(crop_stream(), **SCALED["bilinear_u8_rgb"]) as fr:
        assert len(fr) == 16
    us, n = m2dec_amd.frame_out_timing(reset=True)
    assert n == 16 and us > 0


@pytest.mark.gpu
def test_cuda_array_interface_carries_the_dtype(built):
    with m2dec_amd.decode_to_device(crop_stream(), **SCALED["area_f16_rgbp"]) as fr:
        cai = fr.__cuda_array_interface__
        assert cai["typestr"] == "<f2" and cai["shape"] == (16, 3, 93, 160) == fr.shape and cai["data"] == (fr.ptr, False)
    with m2dec_amd.decode_to_device(crop_stream(), fmt="rgb", size=(8, 8), dtype="f32") as fr:
        assert fr.__cuda_array_interface__["typestr"] == "<f4" and fr.numpy().dtype == np.float32
    with m2dec_amd.decode_to_device(crop_stream(), fmt="rgb", size=(8, 8)) as fr:
        assert fr.__cuda_array_interface__["typestr"] == "|u1" and fr.numpy().dtype == np.uint8


TORCH_CODE = """
import torch
torch.cuda.init()  # torch's HIP runtime is the process's one copy: loaded before the library asks for the same soname
import numpy as np
import m2dec_amd
from tests._frame_out import crop_stream
with m2dec_amd.decode_to_device(crop_stream(), fmt="rgbp", size=(93, 160), filter="area", dtype="f16",
                                mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)) as fr:
    host = fr.numpy()
    t = torch.as_tensor(fr, device="cuda:0")
    assert tuple(t.shape) == fr.shape == (16, 3, 93, 160) and t.dtype == torch.float16 and t.data_ptr() == fr.ptr
    assert host.dtype == np.float16 and t.cpu().numpy().tobytes() == host.tobytes() and host.any()
    del t
print("TORCH_OK")
"""


@pytest.mark.gpu
def test_torch_adopts_the_float16_frames(built):
    """In a process of its own with torch imported first, as test_gpu_frame_out.test_torch_adopts_the_frames."""
    pytest.importorskip("torch")
    r = subprocess.run([sys.executable, "-c", TORCH_CODE], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and r.stdout.strip().endswith("TORCH_OK"), r.stdout[-1000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_neither_tables_nor_mode_leak_into_later_back_ends(built):
    name = "cov_tools_s1"
    with m2dec_amd.decode_to_device(crop_stream(), **SCALED["area_f16_rgbp"]) as fr:
        assert len(fr) == 16
    with m2dec_amd.decode_to_device(stream(name), fmt="nv12") as fr:
        assert fr.shape == (len(GOLDEN[name]["md5"]), 288, 320) and fr.numpy().dtype == np.uint8
        assert _md5s(fr.numpy()) == GOLDEN[name]["md5"]
    with m2dec_amd.decode_to_device(crop_stream(), fmt="nv12") as fr:
        assert _md5s(fr.numpy()) == crop_stream_oracle_md5()
    st = m2dec_amd.Stats()
    assert m2dec_amd.decode_stream_md5(stream(name), stats=st) == GOLDEN[name]["md5"]
    assert st.d2h_bytes == 320 * 192 * 3 // 2 * len(GOLDEN[name]["md5"])
    assert m2dec_amd.decode_stream_md5(crop_stream()) == crop_stream_oracle_md5()
