"""Inputs of the dataset-tool fixtures (tests/golden/segment_dataset.npz, dataset_preprocessor.npz):
built here from seeds, so the fixture generator (tools/make_golden_dataset.py, which runs the
reference modules on them) and the tests (tests/test_dataset_tools.py) see the same data.  The
fixtures pin them by SHA-256.
"""
import hashlib
import json
import os

import numpy as np

# ---------------------------------------------------------------------------- ProbeSegmenter
SEGMENTER_SETTINGS = {
    "default": {},
    # sharp_idx = int(len * 1.0) = len and blurry_idx = len: both thresholds fall back to 0
    "idx_at_len": {"blur_sharp_percentile": 0.0, "blur_blurry_percentile": 100.0},
    "other": {"pose_easy_threshold": 10.0, "pose_medium_threshold": 25.0, "face_large_threshold": 120,
              "face_medium_threshold": 60, "blur_sharp_percentile": 30.0, "blur_blurry_percentile": 40.0,
              "det_score_threshold": 0.5},
}


def metadata_list(n=300, seed=0xFACE5E6):
    """n entries with DatasetPreprocessor's keys: seeded values, then hand-built ones exactly on every
    threshold of the default settings, and entries with keys missing."""
    r = np.random.Generator(np.random.PCG64(seed))
    out = []
    for i in range(n):
        out.append({
            "filename": f"c{i % 7:02d}_{('center', 'left', 'right')[i % 3]}_{i:03d}_face{i % 2}.jpg",
            "class_id": f"c{i % 7:02d}", "source_image": f"IMG_{i:04d}.png",
            "standardized_name": f"c{i % 7:02d}_{('center', 'left', 'right')[i % 3]}_{i:03d}.jpg",
            "face_index": i % 2, "angle": ("center", "left", "right")[i % 3],
            "det_score": float(r.uniform(0.3, 1.0)), "yaw": float(r.normal(0, 20)), "pitch": float(r.normal(0, 12)),
            "roll": float(r.normal(0, 8)), "blur_score": float(r.gamma(2.0, 150.0)),
            "face_size": int(r.integers(20, 260)), "bbox": [int(x) for x in r.integers(0, 1000, 4)],
        })
    # exactly on the thresholds: pose 15 = (9, 12), pose 30 = (18, 24) (exact square roots), sizes 80 and
    # 150, det 0.7; and just past each
    edges = [(9.0, 12.0, 80, 0.7), (-9.0, -12.0, 79, 0.7), (18.0, -24.0, 150, 0.7), (18.0, 24.000001, 149, 0.6999999),
             (9.0, 12.000001, 150, 0.7000001), (0.0, 15.0, 80, 0.5), (30.0, 0.0, 81, 0.4999999), (0.0, 0.0, 0, 1.0)]
    for j, (yaw, pitch, size, det) in enumerate(edges):
        m = dict(out[j])
        m.update(filename=f"edge_{j:02d}_face0.jpg", yaw=yaw, pitch=pitch, face_size=size, det_score=det)
        out.append(m)
    # a blur score equal to another entry's (whichever entry a threshold lands on, its twin is on it too)
    for j in (3, 90, 150, 240):
        m = dict(out[j])
        m["filename"] = f"twin_{j:03d}_face0.jpg"
        out.append(m)
    # missing keys: the .get defaults (yaw / pitch 0, blur 0, det 1.0, size 0)
    for j, drop in enumerate((("yaw",), ("pitch", "yaw"), ("blur_score",), ("det_score",), ("face_size",),
                              ("yaw", "pitch", "blur_score", "det_score", "face_size", "roll"))):
        m = {k: v for k, v in out[10 + j].items() if k not in drop}
        m["filename"] = f"missing_{j:02d}_face0.jpg"
        out.append(m)
    return out


def segment_run_list():
    """The (smaller) list of the recorded segment_dataset run and the files of its input directory:
    every entry's file under its own name, except one present only under a longer name that ends with
    it and one with no file at all."""
    full = metadata_list()
    picked = full[:24] + full[300:]  # seeded entries, the edges, twins and missing-key entries
    files = {}
    for i, m in enumerate(picked):
        if i == 5:
            files["labeled_S017_" + m["filename"]] = i
        elif i == 9:
            continue
        else:
            files[m["filename"]] = i
    files["stray_without_metadata.jpg"] = 999
    return picked, files


def write_segment_inputs(root, picked, files):
    src = os.path.join(root, "probe_positive")
    os.makedirs(src)
    for name, i in files.items():
        with open(os.path.join(src, name), "wb") as f:
            f.write(b"crop %d\n" % i)
    meta = os.path.join(root, "probe_positive_metadata.json")
    with open(meta, "w") as f:
        json.dump(picked, f, indent=2)
    return src, meta


def sha_json(obj) -> str:
    return hashlib.sha256(json.dumps(obj, sort_keys=True).encode()).hexdigest()


# ---------------------------------------------------------------------------- DatasetPreprocessor
# (relative path, first pixel's red value or None for bytes that are no image).  faces_for() returns
# red % 3 faces, so the tree holds photographs with 0, 1 and 2 faces.
TREE = [
    ("class_a/center/b_second.png", 4), ("class_a/center/a_first.PNG", 2), ("class_a/center/notes.txt", None),
    ("class_a/right/r1.bmp", 5), ("class_a/right/r0.png", 3),           # no class_a/left folder
    ("class_b/IMG_left_02.png", 1), ("class_b/img_RIGHT_01.png", 8), ("class_b/portrait.bmp", 7),
    ("class_b/leftright.png", 2), ("class_b/broken.jpeg", None), ("class_b/readme.md", None),
    ("class_c/nothing_here.txt", None),                                  # a class with no images
    ("class_d/left/only_left.png", 10),                                  # a lone angle folder
    ("top_level_file.png", 1),                                           # not a class folder
]
SIZES = [(20, 30), (31, 17), (24, 24)]


def build_tree(root):
    from PIL import Image
    for i, (rel, red) in enumerate(TREE):
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        if red is None:
            with open(path, "wb") as f:
                f.write(b"this is not an image\n")
            continue
        h, w = SIZES[i % len(SIZES)]
        img = np.random.Generator(np.random.PCG64(100 + i)).integers(0, 256, (h, w, 3), dtype=np.uint8)
        img[0, 0, 0] = red
        fmt = {"png": "PNG", "bmp": "BMP"}[rel.rsplit(".", 1)[1].lower()]
        Image.fromarray(img, "RGB").save(path, format=fmt)
    return root


def faces_for(image_rgb, size=224):
    """The stub processor's answer for a decoded photograph: image[0, 0, 0] % 3 faces whose values
    derive from its pixels, in FaceProcessor's result layout (numpy scalar types as the real one has;
    the second face's metrics lack blur_score and roll, as a face rejected before those checks does)."""
    n = int(image_rgb[0, 0, 0]) % 3
    h, w = image_rgb.shape[:2]
    faces = []
    for k in range(n):
        px = image_rgb[min(k + 1, h - 1), min(k + 2, w - 1)].astype(np.int64)
        metrics = {"det_score": float(0.5 + px[0] / 512.0), "face_size": np.int32(40 + px[1] + k),
                   "yaw": np.float32(px[2] / 4.0 - 30.0), "pitch": np.float64(px[0] / 8.0 - 15.0)}
        if k == 0:
            metrics["roll"] = np.float32(px[1] / 16.0 - 8.0)
            metrics["blur_score"] = np.float64(px[2] * 3.25 + h)
        crop = np.empty((size, size, 3), np.uint8)
        crop[...] = (px + 17 * k) % 256
        crop[::7, ::5] = 255 - crop[::7, ::5]
        faces.append({"aligned_face": crop, "bbox": np.array([k, 2 * k, w + k, h + 2 * k], np.int32),
                      "landmarks": np.zeros((5, 2), np.float32), "det_score": metrics["det_score"],
                      "quality_metrics": metrics, "is_valid": k == 0})
    return faces
