"""Identity matching on the GPU: what DESIGN.md §16 "Measured" reports.

    python tools/identities_time.py [--json identities_time.json] [--skip-model]

1. ``fr_match_identities``, the fused kernel (serving tiles of 64, 128 and 256 rows) against the
   composed path (score GEMM + aggregation kernel + top-k), through ``frt_set_identify_path`` /
   ``frt_set_identify_tile_rows``: n in {1, 4, 16} queries, 1,000 and 100,000 identities x 8 rows, the
   three aggregations, top-5.
2. ``fr_embed_match_identities`` against ``fr_embed_match`` at batch 1 on one finalised IR-101 handle
   with 1,000 students (1,000 templates / 1,000 x 8 sample rows).

Every figure is a host clock around a batch of calls that ends in a device synchronise, per call; a
variant's figure is the median of ``--rounds`` (>= 7) such samples after a warm-up, the variants of a
table taken in turn inside every round.  Two variants are measured twice per round under different
names: the difference of their two medians is the spread printed beside every difference.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from facerecognitionpipeline_amd import _lib  # noqa: E402

RULE, FUSED, COMPOSED = 0, 1, 2
AGGS = (("max", 3), ("mean", 3), ("topk", 3))
NS = (1, 4, 16)
TOP = 5


def sample_ms(fn, calls):
    fn()
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / calls * 1e3


def unit_rows(n, seed, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x = torch.randn((n, 512), generator=g, device=dev, dtype=torch.float32)
    return (x / x.norm(dim=1, keepdim=True)).contiguous()


def paths_table(L, dev, n_ids, rows_per_id, rounds, calls):
    h = _lib.Handle("ir_50", "adaface", dev, max_batch=1)
    E = unit_rows(n_ids * rows_per_id, 1, dev)
    offsets = np.arange(n_ids + 1, dtype=np.int32) * rows_per_id
    Q = unit_rows(max(NS), 2, dev)
    # (name, path, tile rows); "again" variants repeat a variant: their distance is the spread
    variants = [("composed", COMPOSED, 0), ("fused64", FUSED, 64), ("fused128", FUSED, 128),
                ("fused256", FUSED, 256), ("composed_again", COMPOSED, 0), ("fused64_again", FUSED, 64)]
    samples = {(v[0], n, a): [] for v in variants for n in NS for a, _k in AGGS}
    bufs = {n: (torch.empty((n, TOP), dtype=torch.int32, device=dev), torch.empty((n, TOP), dtype=torch.float32, device=dev))
            for n in NS}
    cap_set = None
    try:
        for _round in range(rounds):
            for name, path, cap in variants:
                if cap and cap != cap_set:
                    assert L.frt_set_identify_tile_rows(cap) == 0
                    h.samples_set(E, offsets)
                    cap_set = cap
                elif cap_set is None:
                    h.samples_set(E, offsets)
                    cap_set = 64  # the library's default
                assert L.frt_set_identify_path(path) == 0
                for n in NS:
                    q = Q[:n].contiguous()
                    idx, score = bufs[n]
                    for agg, agg_k in AGGS:
                        samples[name, n, agg].append(
                            sample_ms(lambda: h.match_identities(q, agg, agg_k, TOP, idx, score), calls))
    finally:
        L.frt_set_identify_path(RULE)
        L.frt_set_identify_tile_rows(0)
    h.close()
    med = {key: float(np.median(v)) for key, v in samples.items()}
    out = []
    print(f"\n{n_ids} identities x {rows_per_id} rows, top-{TOP}: ms per call, median of {rounds} samples of {calls} calls")
    print(f"{'n':>3} {'agg':>5} {'composed':>9} {'fused64':>9} {'fused128':>9} {'fused256':>9} "
          f"{'f64-comp':>10} {'spread':>8}")
    for n in NS:
        for agg, _k in AGGS:
            spread = max(abs(med["composed", n, agg] - med["composed_again", n, agg]),
                         abs(med["fused64", n, agg] - med["fused64_again", n, agg]))
            row = {"n_ids": n_ids, "rows_per_id": rows_per_id, "n": n, "aggregation": agg, "spread_ms": spread,
                   **{name: med[name, n, agg] for name, _p, _c in variants},
                   "min_max_ms": {name: [float(min(samples[name, n, agg])), float(max(samples[name, n, agg]))]
                                  for name, _p, _c in variants}}
            out.append(row)
            print(f"{n:3d} {agg:>5} {row['composed']:9.4f} {row['fused64']:9.4f} {row['fused128']:9.4f} "
                  f"{row['fused256']:9.4f} {row['fused64'] - row['composed']:+10.4f} {spread:8.4f}", flush=True)
    return out


def batch1_table(dev, rounds, calls, students=1000, rows_per_id=8):
    from facerecognitionpipeline_amd import weights as W
    from facerecognitionpipeline_amd.face_embedder import FaceEmbedder
    emb = FaceEmbedder(architecture="ir_101", model_path="synthetic", max_batch=256)
    h = emb.model
    h.gallery_set(unit_rows(students, 3, dev))
    h.samples_set(unit_rows(students * rows_per_id, 4, dev), np.arange(students + 1, dtype=np.int32) * rows_per_id)
    rgb = torch.from_numpy(W.synthetic_crops(1, seed=9)).to(dev)
    idx = torch.empty((1, 3), dtype=torch.int32, device=dev)
    score = torch.empty((1, 3), dtype=torch.float32, device=dev)
    variants = [("embed_match", lambda: h.embed_match(rgb, 3, idx, score)),
                ("identities_topk", lambda: h.embed_match_identities(rgb, "topk", 3, 3, idx, score)),
                ("identities_max", lambda: h.embed_match_identities(rgb, "max", 3, 3, idx, score)),
                ("identities_mean", lambda: h.embed_match_identities(rgb, "mean", 3, 3, idx, score)),
                ("embed_match_again", lambda: h.embed_match(rgb, 3, idx, score)),
                ("identities_topk_again", lambda: h.embed_match_identities(rgb, "topk", 3, 3, idx, score))]
    samples = {name: [] for name, _fn in variants}
    for _round in range(rounds):
        for name, fn in variants:
            samples[name].append(sample_ms(fn, calls))
    med = {name: float(np.median(v)) for name, v in samples.items()}
    spread = max(abs(med["embed_match"] - med["embed_match_again"]),
                 abs(med["identities_topk"] - med["identities_topk_again"]))
    print(f"\nbatch 1, IR-101, {students} students ({students} templates / {students * rows_per_id} sample rows), top-3: "
          f"ms per call, median of {rounds} samples of {calls} calls; spread of repeated identical runs {spread:.4f} ms")
    for name, _fn in variants:
        print(f"{name:>24} {med[name]:8.4f}  ({med[name] - med['embed_match']:+.4f} against embed_match; "
              f"min {min(samples[name]):.4f} max {max(samples[name]):.4f})", flush=True)
    return {"students": students, "rows_per_id": rows_per_id, "median_ms": med, "spread_ms": spread,
            "min_max_ms": {name: [float(min(v)), float(max(v))] for name, v in samples.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the tables to this file")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--skip-model", action="store_true", help="leave the IR-101 batch-1 table out")
    ap.add_argument("--sizes", default="1000,100000", help="identity counts of the path tables")
    ap.add_argument("--ns", default="1,4,16", help="query counts of the path tables")
    args = ap.parse_args()
    if args.rounds < 7:
        ap.error("--rounds must be at least 7")
    global NS
    NS = tuple(int(x) for x in args.ns.split(","))
    dev = torch.device("cuda", 0)
    L = _lib.load()
    for name in ("frt_set_identify_path", "frt_set_identify_tile_rows"):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int]
    out = {"paths": [], "device": torch.cuda.get_device_name(0), "library": L.fr_version().decode()}
    for n_ids in [int(x) for x in args.sizes.split(",")]:
        out["paths"] += paths_table(L, dev, n_ids, 8, args.rounds, 20 if n_ids <= 10000 else 5)
    if not args.skip_model:
        out["batch1"] = batch1_table(dev, args.rounds, 20)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
