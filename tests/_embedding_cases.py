"""Inputs of the embedding-tool fixture (tests/golden/embedding_tools.npz): the enrollment, probe and
labeler trees, the stub face processor, the host stand-in embedder and the stub gallery, built here
from seeds, so the fixture generator (tools/make_golden_embeddings.py, which runs the reference
``embedding_generator`` / ``probe_labeler`` on them) and the tests (tests/test_embedding_tools.py,
tests/test_gpu_embedding_generator.py) see the same data.  The fixture pins the trees by SHA-256.

Every image file holds PNG bytes whatever its suffix (PIL, like cv2.imread, decodes by content), so
``.jpg`` / ``.jpeg`` names are lossless here too.
"""
import hashlib
import json
import os

import numpy as np

from tests._dataset_cases import faces_for

MODEL_TYPE, ARCHITECTURE = "adaface", "ir_50"
MODEL_NAME = f"{MODEL_TYPE}_{ARCHITECTURE}"
NOT_AN_IMAGE = b"this is not an image\n"

# (path under <dataset_root>/enrollment, first pixel's red value; None: bytes that are no image).  The
# stub processor answers red % 3 faces (faces_for), so: carol's only file has no face, erin's only file
# does not decode (both persons are left out), frank has no listed file at all; dave's .PNG and .bmp are
# not listed (the glob is case-sensitive and knows no .bmp).
ENROLLMENT = [
    ("one-shot/alice/alice_01.png", 1), ("one-shot/bob/bob_01.jpg", 2), ("one-shot/carol/carol_01.png", 3),
    ("one-shot/dave/dave_01.jpeg", 4), ("one-shot/dave/ignored_upper.PNG", 1), ("one-shot/dave/ignored.bmp", 1),
    ("one-shot/erin/broken.png", None), ("one-shot/frank/notes.txt", None), ("one-shot/stray_file.png", 1),
    ("few-shot/alice/a1.png", 7), ("few-shot/alice/a2.jpg", 5), ("few-shot/alice/a3.png", 6),
    ("few-shot/bob/b2.png", 1), ("few-shot/bob/b1.png", 2), ("few-shot/dave/d1.jpeg", 10),
    ("few-shot/dave/broken.jpg", None), ("few-shot/dave/skipped.BMP", 1),
]
PHOTO_SIZES = [(24, 30), (31, 17), (20, 20)]

# (path under <output_root>/probe_labeled, (height, width); None: bytes that are no image).  Crops of
# 224 x 224, 112 x 112 and odd sizes; names with and without a numeric part; two segment folders with
# files, one empty, the other seven absent; negatives with 'lfw' in any letter case, and without.
PROBES = [
    ("positive/alice_001_face0.png", (224, 224)), ("positive/alice_002_face0.jpg", (112, 112)),
    ("positive/bob_smith_003_face0.png", (224, 224)), ("positive/bob_smith_x.png", (150, 130)),
    ("positive/S017_face0.png", (224, 224)), ("positive/001_x.jpg", (112, 112)),
    ("positive/dave_007_face1.jpeg", (224, 224)), ("positive/alice_005_broken.png", None),
    ("positive/alice_009.bmp", (112, 112)), ("positive/alice_010.JPG", (112, 112)),
    ("segmented/high_quality/alice_001_face0.png", (224, 224)), ("segmented/high_quality/dave_002_face0.png", (112, 112)),
    ("segmented/pose_hard/bob_001.png", (97, 113)), ("segmented/pose_hard/bob_002_bad.jpeg", None),
    ("segmented/blur_sharp/readme.txt", None),
    ("negative/stranger_001.png", (224, 224)), ("negative/lfw_George_0001.png", (112, 112)),
    ("negative/Some_LFW_x.jpg", (224, 224)), ("negative/other_002.jpeg", (60, 200)),
    ("negative/unreadable.png", None),
]

# The labeler's probe folder: (name, (height, width) or None, block).  ``block`` goes into the green values
# of the top-left 4 x 4 pixels and selects the 16 dimensions the stand-in embedder writes (fake_embedding), so files of
# different blocks are exactly orthogonal.  listdir order is not sorted order on purpose; .BMP and .Jpeg
# are listed (the labeler lower-cases), .txt is not.
LABELER_PROBES = [
    ("p_07.png", (224, 224), 0), ("p_01.png", (112, 112), 0), ("p_03.jpg", (224, 224), 1),
    ("p_02.BMP", (113, 111), 4), ("p_04_unreadable.png", None, 0), ("p_05.Jpeg", (224, 224), 2),
    ("p_06.png", (112, 112), 3), ("p_08.png", (96, 96), 1), ("notes.txt", None, 0),
]
LABELER_METADATA = [{"filename": "p_01.png", "class_id": "c01", "det_score": 0.75, "bbox": [1, 2, 3, 4]},
                    {"filename": "p_03.jpg", "class_id": "c02", "yaw": -3.5},
                    {"filename": "absent.png", "class_id": "c09"}]
TOP_K = 3


def _pixels(seed, h, w):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _write(path, img):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    if img is None:
        with open(path, "wb") as f:
            f.write(NOT_AN_IMAGE)
    else:
        with open(path, "wb") as f:  # PNG bytes under any suffix
            Image.fromarray(img, "RGB").save(f, format="PNG")


def build_dataset(dataset_root):
    for i, (rel, red) in enumerate(ENROLLMENT):
        img = None
        if red is not None:
            img = _pixels(500 + i, *PHOTO_SIZES[i % len(PHOTO_SIZES)])
            img[0, 0, 0] = red
        _write(os.path.join(dataset_root, "enrollment", rel), img)
    return dataset_root


def build_probes(output_root):
    for i, (rel, size) in enumerate(PROBES):
        _write(os.path.join(output_root, "probe_labeled", rel), None if size is None else _pixels(700 + i, *size))
    return output_root


def labeler_images():
    """name -> pixels of the labeler folder's decodable files."""
    out = {}
    for i, (name, size, block) in enumerate(LABELER_PROBES):
        if size is not None:
            out[name] = _pixels(900 + i, *size)
            out[name][:4, :4, 1] = block  # the resized crop's pixel [0, 0] keeps it
    return out


def build_labeler_probes(folder):
    images = labeler_images()
    for name, _size, _block in LABELER_PROBES:
        _write(os.path.join(folder, name), images.get(name))
    return folder


def sha_json(obj) -> str:
    return hashlib.sha256(json.dumps(obj, sort_keys=True).encode()).hexdigest()


def trees_sha256() -> str:
    return sha_json([ENROLLMENT, PHOTO_SIZES, PROBES, LABELER_PROBES, LABELER_METADATA])


class StubProcessor:
    """FaceProcessor.process_image's contract at output_size 112, answered from the pixels."""

    def process_image(self, image_path, return_all=False):
        assert return_all is True
        from PIL import Image
        try:
            with Image.open(image_path) as im:
                im.load()
                rgb = np.array(im.convert("RGB"), dtype=np.uint8)
        except (OSError, ValueError, SyntaxError):
            raise ValueError(f"Could not load image: {image_path}")
        return faces_for(rgb, size=112)


class BatchStubProcessor(StubProcessor):
    """The same answers through ``process_images(paths, return_all=True, errors="return")``."""

    def __init__(self):
        self.calls = []

    def process_images(self, images, return_all=False, errors="raise"):
        assert return_all is True and errors == "return"
        self.calls.append(len(images))
        out = []
        for p in images:
            try:
                out.append(self.process_image(p, return_all=True))
            except ValueError as e:
                out.append(e)
        return out


# ---------------------------------------------------------------------------- host stand-in embedder
FAKE_DIMS = 16  # non-zero dimensions per embedding (the rest of the 512 are zero: the fixture stays small)
FAKE_BLOCKS = 8


def resize_112(img):
    """cv2.resize(img, (112, 112)) as this project restates it (oracle/scrfd.py)."""
    from oracle.scrfd import resize_linear_u8
    return img if img.shape[:2] == (112, 112) else resize_linear_u8(img, 112, 112)


def fake_embedding(img, normalize=True):
    """A fixed function of the pixels, exact in every step: dimensions [16 b, 16 b + 16), b = the green
    value of pixel [0, 0] of the 112 x 112 crop modulo 8, hold integer sums over 16 pixel sets of it modulo 1021
    as multiples of 2^-10; then one float64 norm and one division."""
    img = resize_112(np.asarray(img))
    block = int(img[0, 0, 1]) % FAKE_BLOCKS
    a = img.astype(np.int64).reshape(-1)
    v = np.zeros(512, np.float64)
    for j in range(FAKE_DIMS):
        part = a[j::FAKE_DIMS]
        v[FAKE_DIMS * block + j] = (int((part * (1 + np.arange(len(part)) % 7)).sum()) % 1021 - 510) / 1024.0
    if normalize:
        v = v / (np.sqrt((v * v).sum()) + 1e-8)
    return v.astype(np.float32)


class FakeEmbedder:
    """Numpy stand-in with the reference's methods and this package's ``embed_images``."""
    max_batch = 4

    def extract_embedding(self, face_image, normalize=True):
        return fake_embedding(face_image, normalize)

    def extract_embeddings_batch(self, face_images, normalize=True, batch_size=32):
        if len(face_images) == 0:
            return np.array([])
        return np.stack([fake_embedding(f, normalize) for f in face_images])

    def embed_images(self, images, normalize=True):
        if len(images) == 0:
            return np.zeros((0, 512), np.float32)
        return self.extract_embeddings_batch(list(images), normalize)


# ---------------------------------------------------------------------------- labeler galleries
STUDENTS = [("S001", "alice"), ("S002", "bob"), ("S003", "carol_ann"), ("S004", "dave")]
F32 = np.float32
# file -> the confidence its own gallery row is built to give, and the label that float must get with
# the class defaults (sure 0.5, unsure 0.4): on each threshold, and the float just under each.  float32
# has no 0.4: F32(0.4) is the float above it (UNSURE), the float under that one is below 0.4 (IMPOSTOR).
ENGINEERED = [("p_01.png", F32(0.5), "SURE"), ("p_03.jpg", F32(0.4), "UNSURE"),
              ("p_05.Jpeg", np.nextafter(F32(0.5), F32(0)), "UNSURE"),
              ("p_06.png", np.nextafter(F32(0.4), F32(0)), "IMPOSTOR")]


class _Record:
    def __init__(self, sid, name, template):
        self.student_id, self.name, self.template_embedding = sid, name, template


class StubGallery:
    """The reference's ``search`` arithmetic (float32 rows, numpy dot, argsort) over fixed template
    rows, with this package's ``search_batch``; ``rows=[]`` is the empty gallery."""

    def __init__(self, rows):
        self.students = {sid: _Record(sid, name, np.asarray(r, np.float32))
                         for (sid, name), r in zip(STUDENTS, rows)}

    def get_all_students(self):
        return self.students

    def search(self, query_embedding, top_k=5):
        if len(self.students) == 0:
            return []
        ids = list(self.students)
        emb = np.vstack([self.students[s].template_embedding for s in ids])
        q = query_embedding / (np.linalg.norm(query_embedding) + 1e-8)
        sims = np.dot(emb, q)
        return [(ids[i], self.students[ids[i]].name, float(sims[i])) for i in np.argsort(sims)[::-1][:top_k]]

    def search_batch(self, queries, top_k=5):
        return [self.search(q, top_k) for q in queries]


def threshold_gallery_rows():
    """One template row per ENGINEERED file: a single non-zero element, at one of the larger elements j
    of that file's query q (the stand-in embedding as ``search`` normalises it), chosen so that the
    float32 product row[j] * q[j] is the target float exactly (the first j, by falling magnitude, for
    which a float within 8 ulps of target / q[j] does that).  Every other term of the dot product is an
    exact zero, so the confidence is that float whatever the summation order; files of other blocks
    score exactly 0 against the row."""
    rows = []
    for name, target, _label in ENGINEERED:
        e = fake_embedding(labeler_images()[name])
        q = (e / (np.linalg.norm(e) + 1e-8)).astype(F32)
        row = None
        for j in np.argsort(-np.abs(q), kind="stable")[:FAKE_DIMS]:
            x = F32(target / q[j])
            cands = [x]
            for _ in range(8):
                cands = [np.nextafter(cands[0], F32(-np.inf))] + cands + [np.nextafter(cands[-1], F32(np.inf))]
            hit = [c for c in cands if F32(c * q[j]) == target]
            if hit:
                row = np.zeros(512, F32)
                row[j] = hit[0]
                break
        assert row is not None, (name, target)
        rows.append(row)
    return rows


# ---------------------------------------------------------------------------- recording and comparing
def pack(obj, arrays, prefix):
    """A pickled dict as a JSON-able structure (key order kept, value types named) with its numpy
    arrays moved into ``arrays`` under ``prefix``-derived names."""
    if isinstance(obj, np.ndarray):
        key = f"{prefix}__{len(arrays)}"
        arrays[key] = obj
        return {"__array__": key, "dtype": str(obj.dtype), "shape": list(obj.shape)}
    if isinstance(obj, dict):
        return {"__dict__": [[k, pack(v, arrays, prefix)] for k, v in obj.items()]}
    if isinstance(obj, list):
        return {"__list__": [pack(v, arrays, prefix) for v in obj]}
    assert obj is None or type(obj) in (str, int, bool, float), type(obj)
    return {"__value__": obj, "type": type(obj).__name__}


def strip_summary(summary):
    """generation_summary.json without its clock and path fields."""
    return {k: v for k, v in summary.items() if k not in ("timestamp", "duration_seconds", "output_directory")}


def strip_labeling(doc, output_dir):
    """labeling_results.json without its clock, and with ``labeled_path`` relative to the output folder."""
    doc = json.loads(json.dumps(doc))
    doc["summary"].pop("timestamp")
    for r in doc["results"]:
        if "labeled_path" in r:
            r["labeled_path"] = os.path.relpath(r["labeled_path"], output_dir)
    return doc


def copied_names(output_dir):
    return {label: sorted(os.listdir(os.path.join(output_dir, label))) for label in ("SURE", "UNSURE", "IMPOSTOR")
            if os.path.isdir(os.path.join(output_dir, label))}


EMBEDDING_OUTPUTS = ["gallery_one-shot_base", "gallery_one-shot_augmented", "gallery_few-shot_base",
                     "gallery_few-shot_augmented", "probe_positive_unsegmented", "probe_positive_segmented",
                     "probe_negative"]


GPU_GALLERY = (("p_01.png", 0.9), ("p_03.jpg", 0.45), ("p_05.Jpeg", 0.6), ("p_06.png", 0.3))


def centred_gallery_rows(embeddings):
    """The GPU labeler test's gallery, from the embeddings of the folder's files (name -> unit float32
    [512]).  The synthetic network maps any two crops to cosines of 0.96 and more, so plain embeddings
    would label every file alike; row k is file k's embedding minus the mean embedding of the folder,
    scaled so that file k scores t_k against it (0.9, 0.45, 0.6 and 0.3: SURE, UNSURE, SURE, IMPOSTOR)
    and the other files a fraction of that.  The generator asserts, on the reference's numbers, the
    margins of every label from 0.5 and 0.4 and of every recorded rank from the next."""
    mean = np.mean([np.asarray(e, np.float64) for e in embeddings.values()], axis=0)
    rows = []
    for name, t in GPU_GALLERY:
        e = np.asarray(embeddings[name], np.float64)
        rows.append((t / float(e @ (e - mean)) * (e - mean)).astype(np.float32))
    return rows
