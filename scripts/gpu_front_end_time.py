"""GPU box: the front-end kernels alone on resident tiles -- the three launches of ``preprocess`` + fused stem against the two of
``front_end_fused`` (``demia_resize_hv_u8x4`` + ``demia_stem_pool_mfma_u8``), device-event times per launch and the bytes per second
of what each launch must move.  Small enough for a counter pass (``rocprofv3 --pmc ... -- python scripts/gpu_front_end_time.py --iters 2``).

    python scripts/gpu_front_end_time.py [--batch 48] [--size 2048] [--iters 20] [--strips 0,16,20,25,32] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from deepemia_amd import _lib, p32, synth  # noqa: E402
from deepemia_amd.engine import PIXEL_MEAN, MaskRCNNEngine  # noqa: E402

COPY_RATE = 6.3e12           # bytes per second a device-to-device copy reaches


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return dict(median_us=t[len(t) // 2], min_us=t[0], max_us=t[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--strips", default="0")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = "cuda:0"
    e = MaskRCNNEngine(synth.random_d2_state_dict(50, 2, seed=0), 50, 2, 0.3, dev, "f16x2")
    lib, b, h, w = e.lib, args.batch, args.size, args.size
    g = torch.Generator(device=dev).manual_seed(1)
    images = torch.randint(0, 256, (b, h, w, 3), generator=g, dtype=torch.uint8, device=dev)
    t = e._resize_tables(h, w)
    nh, nw = t["newh"], t["neww"]
    ph, pw = (nh + 31) // 32 * 32, (nw + 31) // 32 * 32
    st = int(torch.cuda.current_stream().cuda_stream)
    mean = (C.c_float * 3)(*PIXEL_MEAN)
    tmp = torch.empty((b, h, nw, 3), dtype=torch.uint8, device=dev)
    xf = torch.zeros((b, ph + 6, pw + 8, 4), dtype=torch.float32, device=dev)
    xb = torch.zeros((b, ph + 6, pw + 8, 4), dtype=torch.uint8, device=dev)
    outs = [torch.zeros((64 + 2 * b * (ph // 4) * (pw // 4) * 64,), dtype=torch.float16, device=dev) for _ in range(2)]
    metas = [torch.zeros((1, 2), dtype=torch.float32, device=dev) for _ in range(2)]
    s_out = p32.plane_scale(e.stem_bound)

    def resize_h():
        _lib.check(lib.demia_resize_h_u8(_lib.ptr(images), _lib.ptr(tmp), b, h, w, nw, _lib.ptr(t["xm"]), _lib.ptr(t["xs"]), _lib.ptr(t["xk"]), t["ksx"], st), "h")

    def resize_v():
        _lib.check(lib.demia_resize_v_norm(_lib.ptr(tmp), _lib.ptr(xf), b, h, nw, nh, ph, pw, _lib.ptr(t["ym"]), _lib.ptr(t["ys"]), _lib.ptr(t["yk"]), t["ksy"], mean,
                                           _lib.F32, st), "v")

    def resize_hv(strip):
        _lib.check(lib.demia_resize_hv_u8x4(_lib.ptr(images), _lib.ptr(xb), b, h, w, nh, nw, ph, pw, _lib.ptr(t["xm"]), _lib.ptr(t["xs"]), _lib.ptr(t["xk"]), t["ksx"],
                                            _lib.ptr(t["ym"]), _lib.ptr(t["ys"]), _lib.ptr(t["yk"]), t["ksy"], strip, st), "hv")

    def stem_f32():
        _lib.check(lib.demia_stem_pool_mfma(_lib.ptr(xf), _lib.ptr(e.stem_planes), _lib.ptr(e.stem_scale_mfma), _lib.ptr(e.stem_bias), _lib.ptr(outs[0]),
                                            _lib.ptr(metas[0]), b, ph, pw, e.stem_s_in, s_out, 1, 0, st), "stem")

    def stem_u8():
        _lib.check(lib.demia_stem_pool_mfma_u8(_lib.ptr(xb), mean, _lib.ptr(e.stem_planes), _lib.ptr(e.stem_scale_mfma), _lib.ptr(e.stem_bias), _lib.ptr(outs[1]),
                                               _lib.ptr(metas[1]), b, ph, pw, e.stem_s_in, s_out, 1, 0, st), "stem_u8")

    src_bytes, tmp_bytes = images.numel(), tmp.numel()
    plane_bytes = b * (ph // 4) * (pw // 4) * 64 * 4
    need = {"resize_h_u8": src_bytes + tmp_bytes, "resize_v_norm": tmp_bytes + b * nh * nw * 16, "stem_pool_mfma": b * nh * nw * 16 + plane_bytes,
            "resize_hv_u8x4": src_bytes + b * nh * nw * 4, "stem_pool_mfma_u8": b * nh * nw * 4 + plane_bytes}
    rows = {}
    for name, fn in (("resize_h_u8", resize_h), ("resize_v_norm", resize_v), ("stem_pool_mfma", stem_f32)):
        rows[name] = timed(fn, args.iters)
    for strip in [int(s) for s in args.strips.split(",")]:
        rows["resize_hv_u8x4" + (f"[strip={strip}]" if strip else "")] = timed(lambda: resize_hv(strip), args.iters)
    resize_hv(0)
    rows["stem_pool_mfma_u8"] = timed(stem_u8, args.iters)
    torch.cuda.synchronize()
    for name, r in rows.items():
        r["bytes_needed"] = need[name.split("[")[0]]
        r["bytes_per_s"] = r["bytes_needed"] / (r["median_us"] * 1e-6)
        r["share_of_copy_rate"] = r["bytes_per_s"] / COPY_RATE
        print(f"{name:28s} median {r['median_us']:8.1f} us  (min {r['min_us']:.1f}, max {r['max_us']:.1f})  {r['bytes_needed'] / 1e6:7.1f} MB  "
              f"{r['bytes_per_s'] / 1e12:5.2f} TB/s = {100 * r['share_of_copy_rate']:4.1f} % of the copy rate")
    same = torch.equal(outs[0], outs[1]) and torch.equal(metas[0], metas[1])
    res = dict(batch=b, size=args.size, new=(nh, nw), kernels=rows, three_launches_us=sum(rows[k]["median_us"] for k in ("resize_h_u8", "resize_v_norm", "stem_pool_mfma")),
               two_launches_us=rows["resize_hv_u8x4"]["median_us"] + rows["stem_pool_mfma_u8"]["median_us"] if "resize_hv_u8x4" in rows else None,
               planes_and_meta_equal=same)
    print(json.dumps({k: v for k, v in res.items() if k != "kernels"}))
    assert same, "the two front ends gave different planes"
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
