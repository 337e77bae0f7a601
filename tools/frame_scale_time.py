"""Kernel time of the device output's conversion per 1080p frame (m2dec_amd_frame_out_timing: HIP events around each
launch), in three configurations of decode_to_device over the c3_1080p_s1 generator stream:

  full_rgbp            full-size uint8 planar RGB (k_frame_out: the yardstick)
  area_224_f16_rgbp    224 x 224, area filter, float16, ImageNet mean / std (k_frame_scale)
  bilinear_640_f32_rgbp 640 x 640, bilinear, float32 (k_frame_scale)

One line per configuration: microseconds per frame and the implied GB/s over 1.5 cw ch bytes read plus the bytes
written.  Each configuration runs as one child process at a time under its own `timeout`; the first failure ends
the run.

    python tools/frame_scale_time.py [--repeats N] [--limit SECONDS]
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    "full_rgbp": dict(fmt="rgbp"),
    "area_224_f16_rgbp": dict(fmt="rgbp", size=(224, 224), filter="area", dtype="f16", mean=(0.485, 0.456, 0.406),
                              std=(0.229, 0.224, 0.225)),
    "bilinear_640_f32_rgbp": dict(fmt="rgbp", size=(640, 640), filter="bilinear", dtype="f32"),
}
ESIZE = {"u8": 1, "f16": 2, "f32": 4}


def step(name, repeats):
    import m2dec_amd
    from tests._streams import stream
    data = stream("c3_1080p_s1")
    kw = CONFIGS[name]
    with m2dec_amd.decode_to_device(data, **kw) as fr:  # warm: pools, tables, clocks
        n, shape = len(fr), fr.shape
    m2dec_amd.frame_out_timing(reset=True)
    for _ in range(repeats):
        with m2dec_amd.decode_to_device(data, **kw) as fr:
            assert len(fr) == n
    us, launches = m2dec_amd.frame_out_timing(reset=True)
    assert launches == n * repeats, (launches, n, repeats)
    cw, ch = 1920, 1080
    written = shape[1] * shape[2] * shape[3] * ESIZE[kw.get("dtype", "u8")]
    per = us / launches
    print(f"frame_scale_time {name}: {per:.2f} us/frame over {launches} launches, out {shape[1:]} "
          f"{kw.get('dtype', 'u8')}, {(1.5 * cw * ch + written) / per / 1e3:.1f} GB/s "
          f"({1.5 * cw * ch / 1e6:.2f} MB read + {written / 1e6:.2f} MB written)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=150, help="seconds per configuration")
    ap.add_argument("--step", choices=sorted(CONFIGS))
    a = ap.parse_args()
    if a.step:
        step(a.step, a.repeats)
        return 0
    for name in CONFIGS:
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--step", name,
                            "--repeats", str(a.repeats)], cwd=ROOT)
        if r.returncode:
            print(f"frame_scale_time: {name} ended with status {r.returncode}: stopping", flush=True)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
