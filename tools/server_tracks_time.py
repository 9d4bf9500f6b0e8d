#!/usr/bin/env python3
"""Time the server-session path, HIP events around each call, medians of
alternating runs after a warm-up of every shape:

* ``fr_server_tracks`` alone (staging, launch, read-back of the track records) on a log of 16
  sessions of 40 tracks of 20..200 appearances;
* a recorded classroom log (60 requests of 30 client tracks, half of them enrolled) through
  ``FaceRecognitionServer.process_requests``, through this module's per-request ``process_faces``
  loop, and through the reference-shaped loop: the same attempts, one ``extract_embedding`` + one
  ``gallery.search(top_k=3)`` each, which is what the parent commit offers a caller.

Synthetic weights, so the scores mean nothing; the log is built so that enrolled tracks are recognised
at once and the others run through their cooldown cycles.  Prints each figure and writes them to
``out.json``.  Usage: ``python tools/server_tracks_time.py [ir_50|ir_101] [out.json]``"""
import base64
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from facerecognitionpipeline_amd.face_embedder import FaceEmbedder  # noqa: E402
from facerecognitionpipeline_amd.face_recognition_server import (FaceRecognitionServer, decode_image,  # noqa: E402
                                                                 encode_png)
from facerecognitionpipeline_amd.gallery_manager import GalleryManager  # noqa: E402
from tests._server_cases import random_tracks  # noqa: E402

N_REQUESTS, N_TRACKS, STEP = 60, 30, 0.5
THRESHOLD = 0.99


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def classroom_log(seed):
    """Requests of 30 client tracks, each a fixed noise crop (so an enrolled track scores 1.0)."""
    r = np.random.Generator(np.random.PCG64(seed))
    crops = r.integers(0, 256, (N_TRACKS, 112, 112, 3), dtype=np.uint8)
    pngs = [encode_png(c) for c in crops]
    requests = []
    for k in range(N_REQUESTS):
        faces = [{"track_id": t, "bbox": [0.0, 0.0, 112.0, 112.0], "det_score": float(r.choice([0.55, 0.7, 0.9])),
                  "quality_metrics": {"blur_score": float(r.choice([60.0, 120.0, 300.0]))},
                  "aligned_face_base64": pngs[t]} for t in range(N_TRACKS) if r.random() < 0.8]
        requests.append({"faces": faces, "frame_count": k + 1})
    return crops, requests


def main():
    arch = sys.argv[1] if len(sys.argv) > 1 else "ir_101"
    emb = FaceEmbedder(architecture=arch, model_path="synthetic", max_batch=256)
    res = {"arch": arch}
    # ---- the launch alone
    r = np.random.Generator(np.random.PCG64(16))
    lengths = r.integers(20, 201, 16 * 40).tolist()
    metrics, clock, order, offsets = random_tracks(16, lengths)
    dev = [torch.from_numpy(x).to(emb.device) for x in (metrics, clock, order)]
    launch = lambda: emb.model.server_tracks(*dev, offsets, 3, 10, 10.0, 0.6)
    launch()
    ms = [event_ms(launch)[0] for _ in range(21)]
    res["launch"] = {"tracks": len(lengths), "detections": int(offsets[-1]), "ms": ms,
                     "median_ms": statistics.median(ms)}
    print("launch", res["launch"]["tracks"], "tracks", res["launch"]["detections"], "detections: median",
          res["launch"]["median_ms"], "ms", flush=True)
    # ---- a classroom log three ways
    crops, requests = classroom_log(7)
    tmp = tempfile.mkdtemp(prefix="server_time_")
    gm = GalleryManager(gallery_path=os.path.join(tmp, "students.npz"), device=emb.device, verbose=False)
    enrolled = emb.extract_embeddings_batch(list(crops[::2]))
    noise = np.random.Generator(np.random.PCG64(8)).standard_normal((35, 512)).astype(np.float32)
    noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    for i, t in enumerate(list(enrolled) + list(noise)):
        gm.add_student(f"S{i:03d}", f"Student {i}", t)
    clocks = [STEP * i for i in range(N_REQUESTS)]
    runs = [0]

    def server():
        runs[0] += 1
        now = [0.0]
        srv = FaceRecognitionServer(similarity_threshold=THRESHOLD, output_dir=tmp, session_name=f"run_{runs[0]}",
                                    processor=object(), embedder=emb, gallery=gm, clock=lambda: now[0], verbose=False)
        return srv, now

    def batched():
        srv, _now = server()
        srv.process_requests(requests, clocks)
        return srv

    def loop():
        srv, now = server()
        for request, c in zip(requests, clocks):
            now[0] = c
            srv.process_faces(request["faces"], request["frame_count"])
        return srv

    first = batched()
    attempts = first.total_recognition_attempts
    with open(os.path.join(first.session_dir, "attendance.json")) as f:
        attendance = json.load(f)
    res["log"] = {"requests": N_REQUESTS, "faces": sum(len(q["faces"]) for q in requests), "attempts": attempts,
                  "recognized": len(attendance["recognized"]), "unrecognized": len(attendance["unrecognized"])}
    print("log", res["log"], flush=True)
    assert loop().total_recognition_attempts == attempts
    # the reference-shaped loop: the same attempts, one batch-1 embed and one search each
    flat = [f for q in requests for f in q["faces"]]
    picked = [flat[i % len(flat)] for i in range(attempts)]

    def batch_one():
        for face in picked:
            crop = decode_image(base64.b64decode(face["aligned_face_base64"]))
            gm.search(emb.extract_embedding(crop, normalize=True), top_k=3)

    batch_one()
    t = {"process_requests": [], "process_faces_loop": [], "embed_search_per_attempt": []}
    for _ in range(5):
        t["process_requests"].append(event_ms(batched)[0])
        t["process_faces_loop"].append(event_ms(loop)[0])
        t["embed_search_per_attempt"].append(event_ms(batch_one)[0])
    for name, ms in t.items():
        res[name] = {"ms": ms, "median_ms": statistics.median(ms)}
        print(name, "median", res[name]["median_ms"], "ms", [round(x, 1) for x in ms], flush=True)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
