#!/usr/bin/env python3
"""Time a list of 2,048 host crops through ``FaceEmbedder.embed_images`` (one ``fr_embed_images`` call)
and through ``extract_embeddings_batch`` (one upload, one resize launch and one scatter per crop size),
all crops 224x224 and five sizes mixed: three alternating runs each, after one warm-up of both; the
``fr_resize_images`` call alone on device-resident crops; and the per-file ``extract_embedding`` loop
over 256 files.  Prints each figure and writes them to ``--out``.
Usage: ``python tools/embed_images_time.py [ir_50|ir_101] [out.json]``"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from facerecognitionpipeline_amd.face_embedder import FaceEmbedder  # noqa: E402

N = 2048
MIXED = [(224, 224), (112, 112), (160, 160), (200, 180), (96, 128)]


def crops(sizes, n, seed):
    r = np.random.Generator(np.random.PCG64(seed))
    return [r.integers(0, 256, size=sizes[i % len(sizes)] + (3,), dtype=np.uint8) for i in range(n)]


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def main():
    arch = sys.argv[1] if len(sys.argv) > 1 else "ir_101"
    emb = FaceEmbedder(architecture=arch, model_path="synthetic", max_batch=256)
    res = {"arch": arch, "n": N}
    for label, sizes in (("one_size_224", MIXED[:1]), ("five_sizes", MIXED)):
        lst = crops(sizes, N, 7)
        new = lambda: emb.embed_images(lst, normalize=True).cpu().numpy()
        old = lambda: emb.extract_embeddings_batch(lst, normalize=True)
        a, b = new(), old()  # warm-up: kernels loaded, tables built
        res[label + "_max_abs_diff"] = float(np.abs(a - b).max())
        t_new, t_old = [], []
        for _ in range(3):
            t_new.append(timed(new)[0])
            t_old.append(timed(old)[0])
        res[label] = {"embed_images_s": t_new, "extract_embeddings_batch_s": t_old,
                      "embed_images_median_s": statistics.median(t_new),
                      "extract_embeddings_batch_median_s": statistics.median(t_old)}
        print(label, res[label], flush=True)
        # the size of embed_images' upload pieces (the default is FaceEmbedder.upload_piece_bytes)
        default = emb.upload_piece_bytes
        for mib in (4, 16, 64, 1 << 20):
            emb.upload_piece_bytes = mib << 20
            new()
            res[f"{label}_pieces_{mib}MiB_s"] = [timed(new)[0] for _ in range(3)]
            print(label, "upload pieces of", mib, "MiB:", res[f"{label}_pieces_{mib}MiB_s"], flush=True)
        emb.upload_piece_bytes = default
    # the resize alone, on device-resident crops (HIP events around the call)
    for label, sizes in (("one_size_224", MIXED[:1]), ("five_sizes", MIXED)):
        dev = [torch.from_numpy(c).to(emb.device) for c in crops(sizes, N, 7)]
        out = torch.empty((N, 112, 112, 3), dtype=torch.uint8, device=emb.device)
        emb.model.resize_images(dev, out)
        ms = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            emb.model.resize_images(dev, out)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        res["resize_images_ms_" + label] = ms
        print("resize_images", label, ms, flush=True)
    lst = crops(MIXED[:1], 256, 8)
    emb.extract_embedding(lst[0])
    loop = [timed(lambda: [emb.extract_embedding(c) for c in lst])[0] for _ in range(3)]
    one = [timed(lambda: emb.embed_images(lst).cpu().numpy())[0] for _ in range(3)]
    res["per_file_loop_256"] = {"extract_embedding_loop_s": loop, "loop_median_s": statistics.median(loop),
                                "embed_images_s": one, "embed_images_median_s": statistics.median(one)}
    print("per_file_loop_256", res["per_file_loop_256"], flush=True)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
