#!/usr/bin/env python3
"""What Resize + CenterCrop on the device cost (GPU box only): the preprocessing kernel alone, inside a forward, through the host path,
and the host resize it replaces.  One JSON line per measurement.

    python3 tools/preproc_time.py [--steps K] [--warmup W] [--images N] [--parts kernel,device,host,cpu] [--dtypes f32,bf16]
                                  [--filter bilinear,bicubic] [--sources 375x500,1080x1920]

Sources: N images (default 256) of 375 x 500 and of 1080 x 1920 (8 distinct random images of each size, repeated), R = 256, S = 224.
  kernel  device time of the vithip_images_u8_resize_crop_to_f32 launches alone (events around REPS calls back to back, median of K
          windows after W warm-up windows), alternated in the same process with vithip_images_u8_to_f32 on N pre-resized images; both set
          against their bytes-moved floors (source window read + fp32 write, resp. 5 bytes per element, at 6.3 TB/s of HBM);
          --filter bilinear,bicubic adds a leg "resize_crop_bicubic" (vithip_images_u8_resize_crop_to_f32_filter, Pillow's BICUBIC) to
          the same alternation and checks its bits against tests/preproc_filter_model.py; the bilinear leg always goes through the
          entry without a filter, so that VIT_HIP_LIBRARY may name an earlier build (A/B timing of the bilinear kernel);
  device  vit_engine_forward_device_images against vit_engine_forward_device_u8 on the pre-resized bytes, ViT-B/16, per dtype: what
          share of a step the preprocessing is.  The two must give the same bits (checked);
  host    vit_engine_forward_host_images on the full-size sources against vit_engine_forward_host_u8 on the pre-resized bytes (fp32
          engine): what the larger upload costs;
  cpu     Pillow's Image.resize of the same N sources on 16 threads of this box (the work the kernel takes over); "not measured" where
          Pillow is not installed (the numpy restatement is no fair stand-in).
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

R, S, CH = 256, 224, 3
SIZES = {"375x500": (375, 500), "1080x1920": (1080, 1920)}
DISTINCT = 8
REPS = 10
HBM_BPS = 6.3e12  # achievable HBM rate of the MI355X


def window_bytes(h, w, support=1.0):
    """Bytes of the source that the crop's supports touch (rows x columns x channels): the least one read of it moves.  support: the
    filter's, in units of max(scale, 1): 1 bilinear, 2 bicubic."""
    import preproc_model as M
    oh, ow = M.resized_size(h, w, R)
    top, left = M.crop_origin(oh, ow, S)

    def span(inn, out, first):
        if inn == out:
            return S
        scale = inn / out
        sup = support * max(scale, 1.0)
        lo = max(int((first + 0.5) * scale - sup + 0.5), 0)
        hi = min(int((first + S - 1 + 0.5) * scale + sup + 0.5), inn)
        return hi - lo
    return span(h, oh, top) * span(w, ow, left) * CH


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "mean_ms": round(statistics.fmean(ms), 4), "windows": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--parts", default="kernel,device,host,cpu")
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--filter", default="bilinear", help="bilinear | bilinear,bicubic: the legs of the kernel part")
    ap.add_argument("--sources", default=",".join(SIZES), help="which of " + ", ".join(SIZES))
    a = ap.parse_args()
    parts, n = a.parts.split(","), a.images
    filters = a.filter.split(",")
    if "bilinear" not in filters or set(filters) - {"bilinear", "bicubic"}:
        sys.exit("--filter: bilinear or bilinear,bicubic")
    for k in list(SIZES):
        if k not in a.sources.split(","):
            del SIZES[k]

    pkg = importlib.import_module("vision-transformer-opencl_amd")
    B = importlib.import_module("vision-transformer-opencl_amd.binding")
    sys.modules.setdefault("vit_amd", pkg)  # the name the test helpers import the package by
    sys.modules.setdefault("vit_amd.binding", B)
    import preproc_model as M
    L = B.lib()
    cfg = pkg.VIT_B16
    mean, std = B.IMAGENET_MEAN, B.IMAGENET_STD
    m, s = (C.c_float * CH)(*mean), (C.c_float * CH)(*std)
    rng = np.random.default_rng(11)
    distinct = {k: [rng.integers(0, 256, size=(h, w, CH), dtype=np.uint8) for _ in range(DISTINCT)] for k, (h, w) in SIZES.items()}
    resized = {k: np.stack([M.resize_crop(im, R, S) for im in v]) for k, v in distinct.items()}  # what torchvision would hand over
    pick = [i % DISTINCT for i in range(n)]
    u8 = {k: np.ascontiguousarray(v[pick]) for k, v in resized.items()}

    L.vithip_event_create.argtypes = [C.POINTER(C.c_void_p)]
    L.vithip_event_record.argtypes = [C.c_void_p, C.c_void_p]
    L.vithip_event_sync.argtypes = [C.c_void_p]
    L.vithip_event_elapsed_ms.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        B.hip_check(L.vithip_event_create(C.byref(e)), "event_create")

    def device_window(fn, reps):
        """ms per call of `reps` calls back to back on the NULL stream, between two events"""
        B.hip_check(L.vithip_device_sync(), "sync")
        B.hip_check(L.vithip_event_record(ev[0], None), "record")
        for _ in range(reps):
            B.hip_check(fn(), "launch")
        B.hip_check(L.vithip_event_record(ev[1], None), "record")
        B.hip_check(L.vithip_event_sync(ev[1]), "event_sync")
        ms = C.c_float()
        B.hip_check(L.vithip_event_elapsed_ms(C.byref(ms), ev[0], ev[1]), "elapsed")
        return ms.value / reps

    # device copies of the sources: the distinct images once, the records point at them
    dev_src = {k: [B.DeviceArray.from_numpy(im) for im in v] for k, v in distinct.items()}
    triples = {k: [(dev_src[k][j].ptr,) + SIZES[k] for j in pick] for k in SIZES}
    records = {k: B.image_records(t) for k, t in triples.items()}
    d_u8 = {k: B.DeviceArray.from_numpy(v) for k, v in u8.items()}
    d_f32 = B.DeviceArray((n, CH, S, S))
    d_cubic = B.DeviceArray((n, CH, S, S)) if "bicubic" in filters else None

    if "kernel" in parts:
        for k in SIZES:
            legs = {"resize_crop": lambda k=k: L.vithip_images_u8_resize_crop_to_f32(None, records[k], n, d_f32.ptr, S, CH, R, m, s),
                    "u8_to_f32": lambda k=k: L.vithip_images_u8_to_f32(None, d_u8[k].ptr, d_f32.ptr, n, S, CH, m, s)}
            if d_cubic is not None:
                legs["resize_crop_bicubic"] = lambda k=k: L.vithip_images_u8_resize_crop_to_f32_filter(
                    None, records[k], n, d_cubic.ptr, S, CH, R, B.RESIZE_FILTERS["bicubic"], m, s)
            ms = {leg: [] for leg in legs}
            order = list(legs)
            for step in range(a.warmup + a.steps):
                for leg in (order if step % 2 == 0 else order[::-1]):
                    t = device_window(legs[leg], REPS)
                    if step >= a.warmup:
                        ms[leg].append(t)
            assert np.array_equal(d_f32.numpy().view(np.uint32), B.images_u8_to_f32(u8[k], mean, std).view(np.uint32))
            floor = {"resize_crop": n * (window_bytes(*SIZES[k]) + CH * S * S * 4) / HBM_BPS * 1e3, "u8_to_f32": n * CH * S * S * 5 / HBM_BPS * 1e3}
            if d_cubic is not None:
                import preproc_filter_model as FM
                want = FM.preprocess(distinct[k], R, S, mean, std, FM.BICUBIC)[pick]
                assert np.array_equal(d_cubic.numpy().view(np.uint32), want.view(np.uint32))
                floor["resize_crop_bicubic"] = n * (window_bytes(*SIZES[k], support=2.0) + CH * S * S * 4) / HBM_BPS * 1e3
            for leg in order:
                med = statistics.median(ms[leg])
                print(json.dumps(dict({"part": "kernel", "source": k, "images": n, "leg": leg, "calls_per_window": REPS,
                                       "bytes_floor_ms": round(floor[leg], 4), "over_bytes_floor": round(med / floor[leg], 2)}, **stats(ms[leg]))),
                      flush=True)
            print(json.dumps({"part": "kernel", "source": k, "resize_crop_over_u8_to_f32": round(statistics.median(ms["resize_crop"]) /
                                                                                                statistics.median(ms["u8_to_f32"]), 2)}), flush=True)
            if d_cubic is not None:
                print(json.dumps({"part": "kernel", "source": k, "bicubic_over_bilinear": round(
                    statistics.median(ms["resize_crop_bicubic"]) / statistics.median(ms["resize_crop"]), 2)}), flush=True)

    def host_timed(fn, sync):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return 1e3 * (time.perf_counter() - t0)

    W = pkg.synth.make_weights(cfg, 1234) if ("device" in parts or "host" in parts) else None
    for dtype in a.dtypes.split(","):
        if W is None:
            break
        eng = B.Engine(cfg, max_batch=n, dtype=dtype)
        eng.load_weights(W)
        d_out = {leg: B.DeviceArray((n, cfg.num_classes)) for leg in ("images", "u8")}
        for k in SIZES:
            if "device" in parts:
                legs = {"images": lambda k=k: eng.forward_device_images(triples[k], d_out["images"].ptr, R, mean, std),
                        "u8": lambda k=k: eng.forward_device_u8(d_u8[k].ptr, n, d_out["u8"].ptr, mean, std)}
                ms = {leg: [] for leg in legs}
                order = list(legs)
                for step in range(a.warmup + a.steps):
                    for leg in (order if step % 2 == 0 else order[::-1]):
                        t = host_timed(legs[leg], eng.sync)
                        if step >= a.warmup:
                            ms[leg].append(t)
                same = bool(np.array_equal(d_out["images"].numpy().view(np.uint32), d_out["u8"].numpy().view(np.uint32)))
                for leg in order:
                    print(json.dumps(dict({"part": "device", "dtype": dtype, "source": k, "images": n, "leg": leg}, **stats(ms[leg]))), flush=True)
                d = statistics.median(ms["images"]) - statistics.median(ms["u8"])
                print(json.dumps({"part": "device", "dtype": dtype, "source": k, "images_minus_u8_ms": round(d, 3),
                                  "share_of_u8_step": round(d / statistics.median(ms["u8"]), 4), "bitwise_equal": same}), flush=True)
                if not same:
                    sys.exit(f"{dtype} {k}: the _images and _u8 probabilities differ")
            if "host" in parts and dtype == "f32":
                src = [distinct[k][j] for j in pick]
                out = {}
                legs = {"images": lambda: out.__setitem__("images", eng.forward_images(src, R, mean, std)),
                        "u8": lambda k=k: out.__setitem__("u8", eng.forward_u8(u8[k], mean, std))}
                ms = {leg: [] for leg in legs}
                order = list(legs)
                steps = max(a.steps // 2, 1)
                for step in range(2 + steps):
                    for leg in (order if step % 2 == 0 else order[::-1]):
                        t = host_timed(legs[leg], eng.sync)
                        if step >= 2:
                            ms[leg].append(t)
                same = bool(np.array_equal(out["images"].view(np.uint32), out["u8"].view(np.uint32)))
                for leg in order:
                    nbytes = n * (SIZES[k][0] * SIZES[k][1] * CH if leg == "images" else S * S * CH)
                    print(json.dumps(dict({"part": "host", "dtype": dtype, "source": k, "images": n, "leg": leg, "input_bytes": nbytes},
                                          **stats(ms[leg]))), flush=True)
                print(json.dumps({"part": "host", "dtype": dtype, "source": k, "bitwise_equal": same, "images_over_u8": round(
                    statistics.median(ms["images"]) / statistics.median(ms["u8"]), 3)}), flush=True)
        eng.close()

    if "cpu" in parts:
        try:
            from PIL import Image
        except ImportError:
            print(json.dumps({"part": "cpu", "result": "not measured: Pillow is not installed on this box"}), flush=True)
            return
        from concurrent.futures import ThreadPoolExecutor
        for k, (h, w) in SIZES.items():
            oh, ow = M.resized_size(h, w, R)
            pil = [Image.fromarray(distinct[k][j]) for j in pick]
            with ThreadPoolExecutor(16) as pool:
                ms = []
                for step in range(2 + 5):
                    t0 = time.perf_counter()
                    list(pool.map(lambda im: im.resize((ow, oh), Image.BILINEAR), pil))
                    if step >= 2:
                        ms.append(1e3 * (time.perf_counter() - t0))
            print(json.dumps(dict({"part": "cpu", "source": k, "images": n, "threads": 16, "what": "Pillow resize only"}, **stats(ms))), flush=True)


if __name__ == "__main__":
    main()
