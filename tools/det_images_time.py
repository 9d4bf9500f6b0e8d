#!/usr/bin/env python3
"""Time a folder's worth of photographs of mixed sizes through detect -> align -> blur (-> match):

  --mode loop          per image: ``FaceDetector.detect`` + ``FaceAligner.align_batch`` +
                       ``FaceQualityFilter.compute_blur_scores`` (what ``FaceProcessor.process_numpy``
                       launches; the only way before ``fr_detect_images``), with a detector of
                       ``max_frames`` 32.
  --mode batch         one ``FaceProcessor.process_images(return_all=True)`` call over all of them (the
                       host route: ``fr_detect_images`` / ``fr_align_images``, host fit, Python gate).
  --mode device        the same call with ``gate="device"`` (``device_chain_images``:
                       ``fr_detect_images_device`` / ``fr_align_images_device``, the gate on the device).
  --mode match         one ``FaceMatcher.match_images`` call (IR-50, a gallery of 16 random rows).
  --mode match_device  the same with ``device_chain=True``.
  --first              ``return_all=False`` for batch / device: one face per photograph comes back.

loop, batch and match use nothing newer than the calls they name, so they also run on an older build
of the library (``FRHIP_LIB=<path to its libfrhip.so>``): that is how a mode of this tree is compared
with the parent commit's build.

32 host-resident images: the nine sizes of tests/test_gpu_image_batches.py cycled, noise of seed 0, the
seeded synthetic SCRFD-10G weights, output size 224, a gate that lets everything through.  Each
repetition is a host clock around work that ends in the calls' own stream synchronisations (every mode
returns host results); ``--warmup`` repetitions first.  Prints one JSON line: the median, the minimum
and the spread of the repetitions in ms, the number of faces and the library's build id.  Run the modes
in processes of their own, alternating, on an otherwise idle device ("Mixed-size image
batches" and §20).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [(1080, 1920), (481, 367), (37, 53), (640, 640), (720, 1280), (600, 1400), (1, 1), (2, 3), (333, 1001)]


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mode", choices=["loop", "batch", "device", "match", "match_device"], required=True)
    ap.add_argument("--first", action="store_true", help="return_all=False (batch / device)")
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args(argv)

    import torch
    from facerecognitionpipeline_amd import _lib
    from facerecognitionpipeline_amd.detector_arch import synthetic_detector_state_dict
    from facerecognitionpipeline_amd.face_recognition import FaceDetector, FaceProcessor

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a CPU run cannot give these times")
    if args.mode in ("loop", "batch", "match"):  # an older build lacks the newer entry points, which these never call
        import ctypes
        old = ctypes.CDLL(_lib.LIB_PATH)
        for name in [n for n in _lib._SIGNATURES if not hasattr(old, n)]:
            del _lib._SIGNATURES[name]
    r = np.random.default_rng(0)
    images = [r.integers(0, 256, (*SIZES[i % len(SIZES)], 3), dtype=np.uint8) for i in range(args.images)]
    det = FaceDetector(state_dict=synthetic_detector_state_dict(), max_frames=32)
    fp = FaceProcessor(output_size=224, detector=det, quality_filter_config={"min_det_score": 0.0, "min_face_size": 0,
                                                                             "max_yaw": 360, "max_pitch": 1e9,
                                                                             "max_roll": 360, "blur_threshold": 0})

    def loop():
        n = 0
        for im in images:
            try:
                faces = det.detect(im)
            except ValueError:  # fr_detect takes no side below 2: the 1x1 image is left out of the loop
                continue
            if not faces:
                continue
            frame = torch.from_numpy(im).to(fp.aligner._ops.device)
            crops = fp.aligner.align_batch(frame, np.stack([f["landmarks"] for f in faces]))
            fp.quality_filter.compute_blur_scores(crops)
            crops.cpu()
            n += len(faces)
        return n

    def batch():
        return sum(len(x) for x in fp.process_images(images, return_all=not args.first))

    def device():
        return sum(len(x) for x in fp.process_images(images, return_all=not args.first, gate="device"))

    if args.mode.startswith("match"):
        import tempfile
        from facerecognitionpipeline_amd.face_embedder import FaceEmbedder
        from facerecognitionpipeline_amd.face_matcher import FaceMatcher
        from facerecognitionpipeline_amd.gallery_manager import GalleryManager
        emb = FaceEmbedder(architecture="ir_50", model_path="synthetic", max_batch=256)
        gm = GalleryManager(gallery_path=os.path.join(tempfile.mkdtemp(), "students.npz"), device=emb.device,
                            verbose=False)
        rows = np.random.default_rng(5).standard_normal((16, 512)).astype(np.float32)
        for i, e in enumerate(rows / np.linalg.norm(rows, axis=1, keepdims=True)):
            gm.add_student(f"S{i}", f"N{i}", e)
        fm = FaceMatcher(similarity_threshold=0.5, architecture="ir_50", embedder=emb, gallery=gm, verbose=False)
        fm.processor = fp

    def match():
        kw = {"device_chain": True} if args.mode == "match_device" else {}
        return sum(r["num_faces"] for r in fm.match_images(images, top_k=3, **kw))

    run = {"loop": loop, "batch": batch, "device": device, "match": match, "match_device": match}[args.mode]
    for _ in range(args.warmup):
        faces = run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        faces = run()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = np.array(ms)
    print(json.dumps({"mode": args.mode + ("_first" if args.first else ""), "images": args.images,
                      "faces": int(faces), "reps": args.reps,
                      "median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(ms.min()), 3),
                      "max_ms": round(float(ms.max()), 3), "version": _lib.load().fr_version().decode()}))


if __name__ == "__main__":
    main()
