"""Photograph roll call on the GPU: what DESIGN.md §17 "Measured" reports.

    python tools/rollcall_time.py [--json rollcall_time.json] [--skip-photographs]

1. ``fr_photo_rollcall`` alone, k = 5, threshold 0.35: 1 photograph of 40 faces and 32 of 60 (a
   classroom: every face's top-1 is its own row, a tenth of the faces share their top-1 with another),
   and 1 photograph of 1,024 faces all-distinct (1,024 grants, nobody looks twice), all wanting the
   same five rows in the same order (5 grants, everybody looks again after each) and as one
   displacement chain (1,024 grants, each pushing the next face to its second row).  Every shape in
   both modes: FR_ROLLCALL_INDEPENDENT runs no round, so the difference is the round loop.  A call
   stages its offsets and synchronises; the figure is the host clock around a batch of calls, per
   call, and beside it the device time between two events around one call.
2. ``FaceMatcher.match_images`` on 32 noise photographs of four sizes against the two-step route
   (``FaceProcessor.process_images(return_all=True)`` + ``FaceMatcher.match_faces``) on the same
   photographs, synthetic SCRFD-10G and IR-50 weights, 100 students: medians of three alternating runs.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from facerecognitionpipeline_amd import _lib  # noqa: E402

K = 5
THRESHOLD = 0.35
SIZES = [(540, 960), (481, 367), (720, 1280), (600, 1400)]


def classroom(r, n_images, n_faces):
    """Top-1 = the face's own row at 0.5 .. 0.9 (a tenth of the faces: their neighbour's row), the
    other columns other rows of the class below it."""
    idx = np.empty((n_images * n_faces, K), np.int32)
    score = np.empty((n_images * n_faces, K), np.float32)
    for f in range(n_images * n_faces):
        own = f % n_faces
        if r.random() < 0.1:
            own = (own + 1) % n_faces
        others = r.permutation(np.setdiff1d(np.arange(n_faces), [own]))[:K - 1]
        idx[f] = np.concatenate([[own], others]) + 1_000_000
        score[f] = -np.sort(-np.concatenate([[r.uniform(0.5, 0.9)], r.uniform(0.2, 0.45, K - 1)]))
    return idx, score, np.arange(n_images + 1, dtype=np.int32) * n_faces


def big(kind, n=1024):
    f = np.arange(n)
    if kind == "distinct":
        idx = f[:, None] * K + np.arange(K)[None, :]
        score = 0.9 - 0.0001 * f[:, None] - 0.05 * np.arange(K)[None, :]
    elif kind == "contending":
        idx = np.tile(np.arange(K), (n, 1)) + 7
        score = 0.9 - 0.0001 * f[:, None] - 0.05 * np.arange(K)[None, :]
    else:  # chain: face j wants row j, then row j + 1
        idx = np.stack([np.maximum(f, 1), f + 1] + [2000 + f * K + c for c in range(K - 2)], axis=1)
        score = np.stack([0.9 - 0.0004 * f + 0.0001, 0.9 - 0.0004 * f] + [np.full(n, 0.1)] * (K - 2), axis=1)
        score[0, 0] = 0.95
    return idx.astype(np.int32), score.astype(np.float32), np.array([0, n], np.int32)


def kernel_table(dev, rounds, calls):
    h = _lib.Handle("ir_50", "adaface", dev, max_batch=1)
    r = np.random.default_rng(5)
    shapes = {"1 x 40": classroom(r, 1, 40), "32 x 60": classroom(r, 32, 60), "1 x 1024 distinct": big("distinct"),
              "1 x 1024 contending": big("contending"), "1 x 1024 chain": big("chain")}
    out = []
    print(f"fr_photo_rollcall, k = {K}: us per call; host clock, median of {rounds} samples of {calls} calls "
          "(device time between events around one call, median)")
    print(f"{'shape':>20} {'grants':>7} {'independent':>20} {'exclusive':>20} {'difference':>11}")
    for name, (idx, score, off) in shapes.items():
        di, ds = torch.from_numpy(idx).to(dev), torch.from_numpy(score).to(dev)
        host = {0: [], 1: []}
        device = {0: [], 1: []}
        grants = int(h.photo_rollcall(di, ds, off, THRESHOLD, 1)[2][:, 1].sum())
        for _round in range(rounds):
            for mode in (0, 1):
                h.photo_rollcall(di, ds, off, THRESHOLD, mode)
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(calls):
                    h.photo_rollcall(di, ds, off, THRESHOLD, mode)
                torch.cuda.synchronize()
                host[mode].append((time.perf_counter() - t) / calls * 1e6)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                h.photo_rollcall(di, ds, off, THRESHOLD, mode)
                b.record()
                b.synchronize()
                device[mode].append(a.elapsed_time(b) * 1e3)
        med = {m: float(np.median(host[m])) for m in host}
        dmed = {m: float(np.median(device[m])) for m in device}
        out.append({"shape": name, "grants": grants, "host_us": med, "device_us": dmed,
                    "host_min_max_us": {m: [float(min(v)), float(max(v))] for m, v in host.items()}})
        print(f"{name:>20} {grants:7d} {med[0]:10.1f} ({dmed[0]:7.1f}) {med[1]:10.1f} ({dmed[1]:7.1f}) "
              f"{med[1] - med[0]:+11.1f}", flush=True)
    h.close()
    return out


def photographs_table(dev, runs=3, n_photos=32, students=100):
    from facerecognitionpipeline_amd.detector_arch import synthetic_detector_state_dict
    from facerecognitionpipeline_amd.face_embedder import FaceEmbedder
    from facerecognitionpipeline_amd.face_matcher import PHOTO_PROCESSOR_CONFIG, FaceMatcher
    from facerecognitionpipeline_amd.face_recognition import FaceDetector, FaceProcessor
    from facerecognitionpipeline_amd.gallery_manager import GalleryManager
    import tempfile
    det = FaceDetector(state_dict=synthetic_detector_state_dict(), device=dev)
    fp = FaceProcessor(output_size=112, detector=det, device=dev,
                       quality_filter_config=dict(PHOTO_PROCESSOR_CONFIG["quality_filter_config"]))
    emb = FaceEmbedder(architecture="ir_50", model_path="synthetic", max_batch=256, device=dev)
    r = np.random.default_rng(11)
    with tempfile.TemporaryDirectory() as tmp:
        gm = GalleryManager(gallery_path=os.path.join(tmp, "students.npz"), device=emb.device, verbose=False)
        rows = r.normal(size=(students, 512)).astype(np.float32)
        rows /= np.linalg.norm(rows, axis=1, keepdims=True)
        for i, e in enumerate(rows):
            gm.add_student(f"S{i:04d}", f"Student {i}", e)
        fm = FaceMatcher(similarity_threshold=THRESHOLD, architecture="ir_50", embedder=emb, gallery=gm, verbose=False)
        fm.processor = fp
        photos = [r.integers(0, 256, SIZES[i % len(SIZES)] + (3,), dtype=np.uint8) for i in range(n_photos)]

        def one_pass():
            return fm.match_images(photos, top_k=K)

        def two_steps():
            faces = fp.process_images(photos, return_all=True)
            flat = [f["aligned_face"] for fs in faces for f in fs]
            return faces, fm.match_faces(flat, top_k=K)

        n_faces = sum(g["num_faces"] for g in one_pass())  # warm-up of both routes
        two_steps()
        samples = {"match_images": [], "process_images + match_faces": []}
        for _run in range(runs):
            for name, fn in (("match_images", one_pass), ("process_images + match_faces", two_steps)):
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                samples[name].append((time.perf_counter() - t) * 1e3)
    print(f"\n{n_photos} photographs of {len(SIZES)} sizes, {n_faces} faces, {students} students, top-{K}: ms per call, "
          f"median of {runs} alternating runs")
    for name, v in samples.items():
        print(f"{name:>30} {np.median(v):9.2f}  (min {min(v):.2f} max {max(v):.2f})", flush=True)
    return {"photographs": n_photos, "faces": n_faces, "students": students,
            "median_ms": {n: float(np.median(v)) for n, v in samples.items()}, "samples_ms": samples}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the tables to this file")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--skip-photographs", action="store_true", help="leave the match_images table out")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "library": _lib.load().fr_version().decode(),
           "kernel": kernel_table(dev, args.rounds, args.calls)}
    if not args.skip_photographs:
        out["photographs"] = photographs_table(dev)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
