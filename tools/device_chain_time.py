#!/usr/bin/env python3
"""Time frames in HBM -> (dets, counts, blur) on the host, two ways, and the fit kernel alone:

  --mode host    ``FaceDetector.detect_batch`` + ``FaceAligner.align_batch`` per frame +
                 one ``FaceQualityFilter.compute_blur_scores``: the chain as its callers stitch it from
                 the host-output calls (one detect sync per chunk, host fits and a sync per frame, one
                 blur sync).  Uses nothing newer than those calls, so it also runs on an older build of
                 the library (``FRHIP_LIB=<path to its libfrhip.so>``).
  --mode device  ``detect_device`` -> ``align_device`` -> ``blur_scores_device`` and ONE copy of
                 (blur, dets, counts, ok) to the host.
  --mode fit     the fit kernel alone on 2,048 slots, between two HIP events
                 (``frt_fit_similarity_device``): the tests' landmark sets tiled, 2,048 x the exact
                 template (the loop ends after one iteration) and 2,048 x five equal points (all 2,000).

32 noise frames of 1080 x 1920 (seed 0) resident on the device, the seeded synthetic SCRFD-10G weights
with ``max_frames=32``, ``--max-faces`` slots per frame in both modes, output size 112.  Each repetition
is a host clock around work that ends with its results on the host; ``--warmup`` repetitions first.
Prints one JSON line: the median, the minimum and the maximum of the repetitions in ms, faces per frame
and the library's build id.  Run the two modes in processes of their own, alternating, on an otherwise
idle device.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def fit_times(lib, check, reps):
    from tests import _fit_sets
    lib.frt_fit_similarity_device.restype = ctypes.c_int
    lib.frt_fit_similarity_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 3
    sets = _fit_sets.landmark_sets(112)
    n = 2048
    cases = {"test_sets_tiled": np.ascontiguousarray(np.resize(sets, (n, 5, 2))),
             "exact_template": np.ascontiguousarray(np.broadcast_to(_fit_sets.template(112), (n, 5, 2))),
             "five_equal_points": np.full((n, 5, 2), 321.5, dtype=np.float32)}
    out = {}
    for name, lm in cases.items():
        M, ok, ms = np.empty((n, 6)), np.empty(n, dtype=np.uint8), ctypes.c_float()
        t = []
        for _ in range(reps):
            check(lib.frt_fit_similarity_device(lm.ctypes.data, n, 112, M.ctypes.data, ok.ctypes.data,
                                                ctypes.byref(ms)))
            t.append(ms.value)
        out[name] = {"median_ms": round(float(np.median(t)), 4), "min_ms": round(min(t), 4),
                     "max_ms": round(max(t), 4), "fitted": int(ok.sum())}
    return out


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mode", choices=["host", "device", "fit"], required=True)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--max-faces", type=int, default=128)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args(argv)

    import torch
    from facerecognitionpipeline_amd import _lib
    from facerecognitionpipeline_amd.detector_arch import synthetic_detector_state_dict
    from facerecognitionpipeline_amd.face_recognition import FaceAligner, FaceDetector, FaceQualityFilter

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a CPU run cannot give these times")
    if args.mode == "host":  # an older build lacks the newer entry points, which this mode never calls
        old = ctypes.CDLL(_lib.LIB_PATH)
        for name in [n for n in _lib._SIGNATURES if not hasattr(old, n)]:
            del _lib._SIGNATURES[name]
    version = _lib.load().fr_version().decode()
    if args.mode == "fit":
        print(json.dumps({"mode": "fit", "slots": 2048, "reps": args.reps, "version": version,
                          **fit_times(_lib.load(), _lib.check, args.reps)}))
        return

    F = args.max_faces
    frames = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (args.frames, 1080, 1920, 3),
                                                                 dtype=np.uint8)).cuda()
    det = FaceDetector(state_dict=synthetic_detector_state_dict(), max_frames=32, max_faces=F)
    aligner, quality = FaceAligner(112), FaceQualityFilter()

    def host():
        faces = det.detect_batch(frames)
        crops = [aligner.align_batch(frames[f], np.stack([d["landmarks"] for d in fs]))
                 for f, fs in enumerate(faces) if fs]
        quality.compute_blur_scores(torch.cat(crops))
        return sum(len(fs) for fs in faces)

    def device():
        dets, counts = det.model.detect_device(frames, det.det_thresh, F)
        crops, _, ok = aligner._ops.handle.align_device(frames, dets, counts, 112)
        blur = quality._ops.handle.blur_scores_device(crops.view(-1, 112, 112, 3))
        host = torch.cat([blur.view(torch.uint8), dets.view(-1).view(torch.uint8), counts.view(torch.uint8),
                          ok.view(-1)]).cpu()
        return int(host[-ok.numel():].sum())

    run = host if args.mode == "host" else device
    for _ in range(args.warmup):
        faces = run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        faces = run()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = np.array(ms)
    print(json.dumps({"mode": args.mode, "frames": args.frames, "max_faces": F,
                      "faces_per_frame": round(faces / args.frames, 2), "reps": args.reps,
                      "median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(ms.min()), 3),
                      "max_ms": round(float(ms.max()), 3), "version": version}))


if __name__ == "__main__":
    main()
