#!/usr/bin/env python3
"""Generate ``tests/golden/embedding_tools.npz`` by running the REFERENCE ``embedding_generator`` and
``probe_labeler`` in the build container (beside tools/make_golden_dataset.py, whose stand-ins it
reuses; runs only where the reference checkout exists, never on the GPU box).

The inputs are the seeded trees of ``tests/_embedding_cases.py`` (pinned by SHA-256): enrollment folders
(persons with one and several files, a person whose only file has no face, one whose only file does
not decode, ``.PNG`` / ``.bmp`` files the listing ignores), labelled probe crops (224 x 224, 112 x 112
and odd sizes, names with and without a numeric part, undecodable files, two segment folders, the rest
absent or empty), negatives with and without ``lfw`` in the name, and the labeler's probe folder.

Two runs of each reference class are recorded:

* ``real__*`` -- with the reference ``FaceEmbedder`` on the synthetic ``ir_50`` weights (as
  tools/make_golden.py builds it): the structure of every pickle the reference wrote, its embeddings,
  the key sets of its JSON files; and the reference ``ProbeLabeler`` with the reference
  ``GalleryManager`` over ``_embedding_cases.centred_gallery_rows`` of the reference's own embeddings:
  labels, counts, copied names, top-k ids and scores (margins asserted here).
* ``fake__*`` -- with the host stand-in embedder of ``_embedding_cases`` (a fixed, exact function of
  the pixels): pickles element-wise, every JSON text with timestamps, durations and paths stripped,
  file names written; the labeler against ``threshold_gallery_rows`` (confidences exactly on 0.5 and
  on the float at 0.4, and on the floats just under them -- verified here), with the class defaults and
  with the command line's ``--unsure_threshold 0.3``.

The face processor is ``_embedding_cases.StubProcessor`` (answers from pixels at size 112).  cv2 is
the stand-in of make_golden.py plus ``flip`` / ``getRotationMatrix2D`` / ``warpAffine(BORDER_REPLICATE)``
from ``tests/_augment_ref.py``, a dummy ``GaussianBlur`` (the reference builds all 16 variants before
it slices to 8) and the restated ``resize``.  The file holds data the reference wrote, nothing of its
program text.
Usage: ``python tools/make_golden_embeddings.py``
"""
from __future__ import annotations

import json
import os
import pickle
import sys

import numpy as np

TOOLS = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, TOOLS)
import make_golden as MG  # noqa: E402  (REPO on sys.path; the stand-in module texts)
import make_golden_dataset as MGD  # noqa: E402

from tests import _embedding_cases as EC  # noqa: E402

CV2_EXTRA = '''
RESTATED_RESIZE = True
BORDER_REPLICATE = 1
_warp_constant = warpAffine
def _R():
    sys.path.insert(0, {repo!r})
    from tests import _augment_ref
    return _augment_ref
def flip(img, code):
    assert code == 1
    return _R().flip(img)
def getRotationMatrix2D(center, angle, scale):
    return _R().rotation_matrix(center, angle, scale)
def warpAffine(img, M, dsize, flags=INTER_LINEAR, borderMode=BORDER_CONSTANT, borderValue=0):
    if borderMode == BORDER_REPLICATE:
        assert flags == INTER_LINEAR and tuple(dsize) == (img.shape[1], img.shape[0])
        return _R().warp_affine_replicate(img, M)
    return _warp_constant(img, M, dsize, flags, borderMode, borderValue)
def GaussianBlur(img, ksize, sigma):
    return img.copy()  # entry 14 of the augmentation list: built, then sliced away (8 are kept)
'''


def tree_files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _s, fs in os.walk(root) for f in fs)


def read_outputs(out_dir):
    """The seven pickles (structure + arrays) and JSON documents of one embedding_generator run."""
    arrays, structs, jsons = {}, {}, {}
    for stem in EC.EMBEDDING_OUTPUTS:
        with open(os.path.join(out_dir, stem + ".pkl"), "rb") as f:
            structs[stem] = EC.pack(pickle.load(f), arrays, stem)
        with open(os.path.join(out_dir, stem + ".json")) as f:
            jsons[stem] = json.load(f)
    with open(os.path.join(out_dir, "generation_summary.json")) as f:
        summary = EC.strip_summary(json.load(f))
    return arrays, structs, jsons, summary


def key_sets(doc):
    """The nested key structure of a JSON document (lists of numbers cut to their length)."""
    if isinstance(doc, dict):
        return {k: key_sets(v) for k, v in doc.items()}
    if isinstance(doc, list):
        return ["list", len(doc)] if not doc or not isinstance(doc[0], (dict, list)) else ["rows", len(doc), len(doc[0])]
    return type(doc).__name__


def main() -> None:
    if not os.path.isdir(MG.REF):
        raise SystemExit("reference not present; golden files are generated in the build container only")
    tmp = MGD.stand_ins()
    with open(os.path.join(tmp, "cv2.py"), "a") as f:
        f.write(CV2_EXTRA.format(repo=MG.REPO))
    with open(os.path.join(tmp, "net.py"), "w") as f:
        f.write(MG.NET_SHIM.format(repo=MG.REPO))
    import torch
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    import embedding_generator as ref_eg  # reference modules (cv2 / insightface / net stand-ins)
    import face_embedder as ref_fe
    import gallery_manager as ref_gm
    import probe_labeler as ref_pl
    from facerecognitionpipeline_amd import weights as W

    ckpt = os.path.join(tmp, "ir_50.ckpt")
    W.save_checkpoint(W.synthetic_state_dict(EC.ARCHITECTURE), ckpt)
    with MG.quiet():
        real = ref_fe.FaceEmbedder(architecture=EC.ARCHITECTURE, model_path=ckpt, model_type=EC.MODEL_TYPE,
                                   device=torch.device("cpu"))

    dataset = EC.build_dataset(os.path.join(tmp, "dataset"))
    out = {"trees_sha256": np.array(EC.trees_sha256())}

    def generator(embedder, output_root):
        g = ref_eg.EmbeddingGenerator.__new__(ref_eg.EmbeddingGenerator)  # __init__ would build FaceAnalysis
        g.model_type, g.architecture, g.model_name = EC.MODEL_TYPE, EC.ARCHITECTURE, EC.MODEL_NAME
        g.dataset_root, g.output_root = ref_eg.Path(dataset), ref_eg.Path(output_root)
        g.embedder, g.face_processor = embedder, EC.StubProcessor()
        g.output_dir = g.output_root / "embeddings" / g.model_name
        g.output_dir.mkdir(parents=True, exist_ok=True)
        return g

    import contextlib
    import io
    for tag, embedder in (("real", real), ("fake", EC.FakeEmbedder())):
        root = EC.build_probes(os.path.join(tmp, f"output_{tag}"))
        g = generator(embedder, root)
        with MG.quiet(), contextlib.redirect_stderr(io.StringIO()):  # tqdm bars
            g.generate_all_embeddings()
        arrays, structs, jsons, summary = read_outputs(str(g.output_dir))
        for k, v in arrays.items():
            out[f"{tag}__{k}"] = v
        out[f"{tag}__structs"] = np.array(json.dumps(structs))
        out[f"{tag}__summary"] = np.array(json.dumps(summary))
        out[f"{tag}__files"] = np.array(json.dumps(tree_files(str(g.output_dir))))
        if tag == "real":
            out["real__json_keys"] = np.array(json.dumps({k: key_sets(v) for k, v in jsons.items()}))
        else:
            out["fake__jsons"] = np.array(json.dumps(jsons))
        print(tag, "summary", summary, {k: v.shape for k, v in arrays.items() if k.startswith("probe_neg")})

    # ---- ProbeLabeler
    folder = EC.build_labeler_probes(os.path.join(tmp, "labeler", "probe_positive"))
    meta = os.path.join(tmp, "labeler", "probe_positive_metadata.json")
    with open(meta, "w") as f:
        json.dump(EC.LABELER_METADATA, f, indent=2)
    images = EC.labeler_images()

    def labeler(embedder, rows, sure=0.5, unsure=0.4):
        lab = ref_pl.ProbeLabeler.__new__(ref_pl.ProbeLabeler)  # __init__ loads the registry's checkpoints
        lab.sure_threshold, lab.unsure_threshold = sure, unsure
        lab.model_type, lab.architecture = EC.MODEL_TYPE, EC.ARCHITECTURE
        lab.embedder = embedder
        with MG.quiet():
            lab.gallery = ref_gm.GalleryManager(gallery_path=os.path.join(tmp, f"g{len(os.listdir(tmp))}", "students.pkl"))
            for (sid, name), row in zip(EC.STUDENTS, rows):
                lab.gallery.add_student(sid, name, np.asarray(row, np.float32))
        return lab

    def run(lab, tag, **kw):
        dst = os.path.join(tmp, "labeler", f"out_{tag}")
        with MG.quiet():
            summary = lab.process_probe_directory(folder, output_dir=dst, metadata_file=meta, top_k=EC.TOP_K, **kw)
        with open(os.path.join(dst, "labeling_results.json")) as f:
            doc = EC.strip_labeling(json.load(f), dst)
        summary = dict(summary)
        summary.pop("timestamp")
        assert summary == doc["summary"]
        out[f"labeler__{tag}__doc"] = np.array(json.dumps(doc))
        out[f"labeler__{tag}__copied"] = np.array(json.dumps(EC.copied_names(dst)))
        return doc

    # the stand-in run: confidences exactly on the thresholds and just under them
    rows = EC.threshold_gallery_rows()
    doc = run(labeler(EC.FakeEmbedder(), rows), "fake")
    got = {r["filename"]: (r["confidence"], r["label"]) for r in doc["results"]}
    for name, target, label in EC.ENGINEERED:
        assert got[name] == (float(target), label), (name, got[name], float(target), label)
    assert float(EC.ENGINEERED[0][1]) == 0.5 and float(EC.ENGINEERED[1][1]) >= 0.4 > float(EC.ENGINEERED[3][1])
    doc03 = run(labeler(EC.FakeEmbedder(), rows, unsure=0.3), "fake_cli_0.3")
    assert {r["filename"]: r["label"] for r in doc03["results"]}["p_06.png"] == "UNSURE"
    run(labeler(EC.FakeEmbedder(), rows), "fake_no_copy", copy_files=False)
    with MG.quiet():
        empty = labeler(EC.FakeEmbedder(), []).match_face(images["p_01.png"])
    assert empty == (None, "UNKNOWN", 0.0, "IMPOSTOR", []), empty
    print("labeler fake", doc["summary"]["label_distribution"], "cli 0.3", doc03["summary"]["label_distribution"])

    # the real run: a gallery of the reference's own embeddings, labels with margins
    with MG.quiet():
        emb = {name: real.extract_embedding(img, normalize=True) for name, img in images.items()}
    rows = EC.centred_gallery_rows(emb)
    doc = run(labeler(real, rows), "real")
    margin = 1.0
    for r in doc["results"]:
        scores = [m["score"] for m in r["top_matches"]]
        assert len(scores) == EC.TOP_K
        margin = min([margin, abs(r["confidence"] - 0.5), abs(r["confidence"] - 0.4)]
                     + [a - b for a, b in zip(scores, scores[1:])])
        print("  ", r["filename"], r["label"], [round(s, 4) for s in scores])
    assert margin >= 2e-3, margin  # 200 x the 1e-5 the GPU test allows a score to move
    assert set(doc["summary"]["label_distribution"].values()) != {0} and min(
        doc["summary"]["label_distribution"].values()) >= 1, doc["summary"]["label_distribution"]
    out["labeler__real__gallery_rows"] = np.stack(rows).astype(np.float32)
    print("labeler real", doc["summary"]["label_distribution"], "smallest margin", margin)

    path = os.path.join(MG.OUT, "embedding_tools.npz")
    np.savez_compressed(path, **out)
    print("embedding_tools", len(out), "arrays;", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
