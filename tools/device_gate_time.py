#!/usr/bin/env python3
"""Time frames in HBM -> the list of valid face slots on the host, with the quality gate on the host
or on the device, and the two gate launches alone:

  --mode host    ``RecognitionPipeline.recognize_frames``' default form up to its ``valid`` list:
                 detect_device -> align_device -> blur_scores_device, ONE copy of (blur, dets, counts,
                 ok), then ``FaceQualityFilter.is_valid`` per face in Python.
  --mode device  its ``gate="device"`` form up to the same point: the three calls, ``gate_device``,
                 ONE copy of (stage, metrics, bbox, valid_slots, n_valid, counts), the dicts rebuilt
                 with ``metrics_from_gate``.
  --mode gate    the two launches of ``fr_quality_gate_device`` alone on the chain's outputs, between
                 two HIP events.

32 noise frames of 1080 x 1920 (seed 0) resident on the device, the seeded synthetic SCRFD-10G weights
with ``max_frames=32``, ``--max-faces`` slots per frame, output size 112 (DESIGN.md §18's setup).
``--config default`` is ``FaceQualityFilter()``; ``loose`` lets every face through every test, so
every face pays the pose arithmetic and the blur test (the host loop's worst case).  Each repetition
is a host clock around work that ends with its results on the host; ``--warmup`` repetitions first.
Prints one JSON line: median, minimum and maximum in ms, the faces and valid faces found and the
library's build id.  Run the modes in processes of their own, alternating, on an otherwise idle device.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LOOSE = {"min_det_score": 0.0, "min_face_size": 0, "max_yaw": 1e9, "max_pitch": 1e9, "max_roll": 1e9,
         "blur_threshold": 0}


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mode", choices=["host", "device", "gate"], required=True)
    ap.add_argument("--config", choices=["default", "loose"], default="default")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--max-faces", type=int, default=128)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args(argv)

    import torch
    from facerecognitionpipeline_amd import _lib
    from facerecognitionpipeline_amd.detector_arch import synthetic_detector_state_dict
    from facerecognitionpipeline_amd.face_recognition import (GATE_VALID, FaceAligner, FaceDetector,
                                                              FaceQualityFilter, tensors_to_host)

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a CPU run cannot give these times")
    version = _lib.load().fr_version().decode()
    n, F, S = args.frames, args.max_faces, 112
    frames = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (n, 1080, 1920, 3), dtype=np.uint8)).cuda()
    det = FaceDetector(state_dict=synthetic_detector_state_dict(), max_frames=32, max_faces=F)
    aligner, quality = FaceAligner(S), FaceQualityFilter(**(LOOSE if args.config == "loose" else {}))

    def chain():
        dets, counts = det.model.detect_device(frames, det.det_thresh, F)
        crops, _, ok = aligner._ops.handle.align_device(frames, dets, counts, S)
        blur = quality._ops.handle.blur_scores_device(crops.view(n * F, S, S, 3))
        return dets, counts, ok, blur

    def host():  # pipeline.py recognize_frames, gate="host", up to `valid`
        dets, counts, ok, blur = chain()
        parts = [blur.view(torch.uint8), dets.view(-1).view(torch.uint8), counts.view(torch.uint8), ok.view(-1)]
        h = torch.cat(parts).cpu().numpy()
        cut = np.cumsum([p.numel() for p in parts])
        h_blur = h[:cut[0]].view(np.float64).reshape(n, F)
        h_dets = h[cut[0]:cut[1]].view(np.float32).reshape(n, F, 15)
        h_counts = h[cut[1]:cut[2]].view(np.int32)
        h_ok = h[cut[2]:].reshape(n, F)
        out, valid = [], []
        for f in range(n):
            rows = []
            for i, d in enumerate(det._faces(h_dets[f], min(int(h_counts[f]), F))):
                good, q = quality.is_valid(d, None, float(h_blur[f, i]))
                good = good and bool(h_ok[f, i])
                rows.append({"bbox": d.get("bbox"), "det_score": d["det_score"], "quality_metrics": q,
                             "is_valid": good, "matches": [], "recognized": False})
                if good:
                    valid.append((f, i))
            out.append(rows)
        return sum(len(r) for r in out), len(valid)

    def device():  # pipeline.py _recognize_gated up to the gather
        dets, counts, ok, blur = chain()
        g = quality.gate_device(dets, counts, ok, blur)
        h = tensors_to_host({**{k: g[k] for k in ("stage", "metrics", "bbox", "valid_slots", "n_valid")},
                             "counts": counts})
        out = []
        for f in range(n):
            rows = []
            for i in range(min(int(h["counts"][f]), F)):
                stage = h["stage"][f, i]
                q = quality.metrics_from_gate(stage, h["metrics"][f, i], h["bbox"][f, i])
                rows.append({"bbox": h["bbox"][f, i].copy(), "det_score": q["det_score"], "quality_metrics": q,
                             "is_valid": bool(stage == GATE_VALID), "matches": [], "recognized": False})
            out.append(rows)
        return sum(len(r) for r in out), int(h["n_valid"][0])

    if args.mode == "gate":
        dets, counts, ok, blur = chain()
        g = quality.gate_device(dets, counts, ok, blur)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            quality.gate_device(dets, counts, ok, blur, g)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms = np.array(ms[args.warmup:])
        faces, valid = int(g["frame_offsets"][-1]), int(g["n_valid"][0])
    else:
        run = host if args.mode == "host" else device
        for _ in range(args.warmup):
            faces, valid = run()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            faces, valid = run()
            ms.append((time.perf_counter() - t0) * 1e3)
        ms = np.array(ms)
    print(json.dumps({"mode": args.mode, "config": args.config, "frames": n, "max_faces": F, "faces": faces,
                      "valid": valid, "reps": args.reps, "median_ms": round(float(np.median(ms)), 4),
                      "min_ms": round(float(ms.min()), 4), "max_ms": round(float(ms.max()), 4), "version": version}))


if __name__ == "__main__":
    main()
