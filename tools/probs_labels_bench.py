"""Scoring the network's own class-vector images on the device (fusion.ConfusionMatrix.add_probs, fusion.argmax_labels_device) at
cfg2's resolution -- 1920 x 1080 -- with 19, 40 and 150 classes in float32, float16 and bfloat16, against a ground truth of large
uniform regions and a random one.  16 device-resident images (synth.device_probs) per leg, medians of 7 repeats with min - max.

Legs, per image:
  a  add_probs: label and count in one call (one kernel up to 63 classes, two beyond)
  b  argmax_labels_device (int32), then cm.add on the flattened label image: the two-pass form
  c  a with the option "probs_labels_tiles" at 0: the generic one-lane-per-pixel path
  a16  a with the same ground truth as uint16: the kernel instance for ground truth that is not uint8 (it waits for its ground-truth
     load where it is issued; the uint8 instance keeps it in flight), up to 63 classes
  d  the route without this interface: where torch imports and sees the device, probs.argmax(-1) handed to cm.add ("torch");
     and on the host, one image: copy, np.argmax, np.add.at ("host")
Kernel time is the library's HIP-event profile slots (SMESH_PROF_PROBS_LABELS, plus SMESH_PROF_CONFUSION where k_confusion runs); the
whole call is a host clock around a synchronise, in runs of their own with profiling off.  Needed bytes of leg a:
W H (C itemsize + ground-truth itemsize), against 8 TB/s.
usage: python tools/probs_labels_bench.py [output file, default profiles/probs_labels_bench.json]"""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semantic_meshes_amd import _lib, device, fusion, synth          # noqa: E402

IMAGES, REPS, PEAK = 16, 7, 8.0e12
SLOTS = (1 << _lib.PROF_PROBS_LABELS) | (1 << _lib.PROF_CONFUSION)


def slot_ms(which):
    ms, n = ctypes.c_double(), ctypes.c_uint64()
    _lib.check(_lib.lib().smesh_profile_read(0, which, ctypes.byref(ms), ctypes.byref(n)))
    return ms.value


def timed(run, profiled):
    """Milliseconds per image of `run()` over the IMAGES images: the kernels' (profile slots) or the whole call's (host clock)."""
    lib = _lib.lib()
    _lib.check(lib.smesh_profile_enable(0, SLOTS if profiled else 0))
    _lib.check(lib.smesh_profile_reset(0))
    _lib.synchronize(0)
    t0 = time.perf_counter()
    run()
    _lib.synchronize(0)
    wall = 1e3 * (time.perf_counter() - t0)
    kernels = slot_ms(_lib.PROF_PROBS_LABELS) + slot_ms(_lib.PROF_CONFUSION) if profiled else None
    _lib.check(lib.smesh_profile_enable(0, 0))
    return (kernels if profiled else wall) / IMAGES


def stats(samples):
    return {"median_us": 1e3 * statistics.median(samples), "min_max_us": [1e3 * min(samples), 1e3 * max(samples)]}


def torch_or_none():
    try:
        import torch
        return torch if torch.cuda.is_available() else None
    except Exception:
        return None


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "probs_labels_bench.json")
    cfg = synth.CONFIGS["cfg2"]
    W, H = cfg["width"], cfg["height"]
    N = W * H
    torch = torch_or_none()
    _lib.check(_lib.lib().smesh_profile_sample_every(0, 1))
    result = {"tool": "tools/probs_labels_bench.py", "width": W, "height": H, "images_per_leg": IMAGES, "reps": REPS,
              "roofline_bytes_per_s": PEAK, "torch_route": "measured" if torch is not None else "not measured", "cases": []}
    for C in (19, 40, 150):
        for dtype in ("float32", "float16", "bfloat16"):
            rng = np.random.default_rng(C)
            images = [synth.device_probs(W, H, C, 1000 + k, dtype=dtype) for k in range(IMAGES)]
            kw = {"probs_dtype": "bfloat16"} if dtype == "bfloat16" else {}
            itemsize = 4 if dtype == "float32" else 2
            cm = fusion.ConfusionMatrix(C)
            case = {"classes": C, "dtype": dtype, "needed_bytes_per_image": N * (C * itemsize + 1),
                    "needed_bytes_per_image_with_labels": N * (C * itemsize + 1 + 1), "ground_truth": {}}
            tensors = None
            if torch is not None:
                try:
                    tensors = [torch.from_dlpack(im) for im in images]
                except Exception as e:                     # (a torch build that does not take the capsule: the leg is not measured)
                    case["torch_route_error"] = repr(e)
                    tensors = None
            for kind in ("uniform", "random"):
                if kind == "uniform":       # 8 x 4 blocks of 240 x 270 pixels, one class each
                    g = ((np.arange(W)[:, None] // 240) + 8 * (np.arange(H)[None, :] // 270)) % C
                    gts_host = [np.ascontiguousarray(np.roll(g, k, axis=0).astype(np.uint8)) for k in range(IMAGES)]
                else:
                    gts_host = [rng.integers(0, C, size=(W, H)).astype(np.uint8) for _ in range(IMAGES)]
                gts = [device.to_device(g) for g in gts_host]
                flat_gts = [device.DeviceArray(g.ptr, (N,), np.uint8, 0, owner=g) for g in gts]
                gts16 = [device.to_device(g.astype(np.uint16)) for g in gts_host]

                def leg_a():
                    for im, g in zip(images, gts):
                        cm.add_probs(im, g, **kw)

                def leg_a16():
                    for im, g in zip(images, gts16):
                        cm.add_probs(im, g, **kw)

                def leg_b():
                    for im, g in zip(images, flat_gts):
                        lab = fusion.argmax_labels_device(im, dtype=np.int32, dont_care_label=-1, **kw)
                        cm.add(device.DeviceArray(lab.ptr, (N,), np.int32, 0, owner=lab), g)

                def leg_c():
                    _lib.set_option("probs_labels_tiles", 0)
                    try:
                        leg_a()
                    finally:
                        _lib.set_option("probs_labels_tiles", 1)

                def leg_d():
                    for t, g in zip(tensors, flat_gts):
                        cm.add(t.argmax(-1).to(torch.int32).reshape(-1), g)
                    torch.cuda.synchronize()

                legs = {"a_add_probs": leg_a, "b_argmax_then_add": leg_b, "c_add_probs_generic_path": leg_c}
                if C <= 63:
                    legs["a16_add_probs_uint16_ground_truth"] = leg_a16
                if tensors is not None:
                    legs["d_torch_argmax_then_add"] = leg_d
                matrices, samples = {}, {(name, prof): [] for name in legs for prof in (False, True)}
                for rep in range(REPS + 1):                # (the first round warms up every shape and is dropped)
                    for name, run in legs.items():
                        for prof in (False, True):
                            if name.startswith("d_") and prof:
                                continue                   # (torch's kernel is not in the library's slots)
                            cm.reset()
                            t = timed(run, prof)
                            if rep:
                                samples[(name, prof)].append(t)
                            else:
                                matrices[name] = (cm.get(), cm.ignored)
                m = {}
                for name in legs:
                    m[name] = {"call": stats(samples[(name, False)])}
                    if samples[(name, True)]:
                        m[name]["kernels"] = stats(samples[(name, True)])
                    m[name]["matrix_equals_leg_a"] = bool(np.array_equal(matrices[name][0], matrices["a_add_probs"][0])
                                                          and matrices[name][1] == matrices["a_add_probs"][1])
                k = m["a_add_probs"]["kernels"]["median_us"] * 1e-6
                m["a_add_probs"]["needed_bytes_per_s"] = case["needed_bytes_per_image"] / k
                m["a_add_probs"]["share_of_roofline"] = case["needed_bytes_per_image"] / k / PEAK
                if kind == "random":                       # the host route, one image
                    t0 = time.perf_counter()
                    host = images[0].numpy()
                    if dtype == "bfloat16":
                        host = (host.astype(np.uint32) << np.uint32(16)).view(np.float32)
                    pred = np.argmax(host, axis=-1)
                    M = np.zeros((C, C + 1), np.uint64)
                    np.add.at(M, (gts_host[0], pred), 1)
                    m["d_host_copy_numpy_argmax_add_at"] = {"call_ms_one_image": 1e3 * (time.perf_counter() - t0)}
                    cm.reset()
                    cm.add_probs(images[0], gts[0], **kw)
                    m["d_host_copy_numpy_argmax_add_at"]["matrix_equals_leg_a"] = bool(np.array_equal(cm.get(), M))
                    del host, pred
                case["ground_truth"][kind] = m
                del gts, flat_gts, gts16
            result["cases"].append(case)
            print(json.dumps(case), flush=True)
            del images, tensors, cm
            if torch is not None:
                torch.cuda.empty_cache()
            device.trim()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
